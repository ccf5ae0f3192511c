"""GPU: keystream payload verification (k_verify_keystream and the calls over it).

Expected bytes come only from the C oracle (oracle_c.dgen_fill,
oracle_c.xoshiro_chunks), never from the library's fill.  The expected
VerifyResult comes from numpy (`expect`): the count of differing bytes, the
count of 4 KiB granules per object holding one, and the lowest offset from the
buffer's start.  Every assertion is exact.

Lane paths: a context whose min_lane_draws knob is set plans lanes of exactly
that many draws (rounded up to 512), so 1 MiB DG1 blocks and 2 MiB K2 chunks run
  "one"   2^18 draws per lane: lpc == 1, no jump
  "vec"   8192: DG1 lpc 16, K2 lpc 32, the per-lane vector jump
  "uni"   1024: DG1 lpc 128, K2 lpc 256, the wave-uniform scalar jump
and "auto" is the default plan (small launches spread down to 512-draw lanes).
The kernel has one workgroup shape (1 wave, 64-draw stages).
"""
import functools
import os
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SOAK = max(1, int(os.environ.get("S3DG_FUZZ_SOAK", "1")))   # soak runs: seeds x SOAK

BLK = 4096
MIB = 1 << 20
HOST_CHUNK = 64 << 20          # the host path's staging chunk
PATHS = {"auto": 0, "one": 1 << 18, "vec": 8192, "uni": 1024}
# lane region of a 1 MiB DG1 block on each path, in bytes (8 x draws per lane;
# "auto": a few blocks spread to 512-draw lanes)
DG1_REGION = {"auto": 4096, "one": MIB, "vec": 65536, "uni": 8192}
DG1_SIZES = [1, 7, 12, 16, 4095, 4096, 4097, MIB - 1, MIB, MIB + 3, 2 * MIB + 4100, 3 * MIB + 13]
DEDUPS = [1, 2, 3]
COMPRESS = [1, 2, 3, (3, 2), 8]


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctxs(S, gpu_ctx):
    """One context per lane path (the shared context stays as it is: "auto")."""
    out = {"auto": gpu_ctx}
    for name, draws in PATHS.items():
        if draws:
            c = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
            c.set_keystream_shape(0, min_lane_draws=draws)
            c.set_keystream_shape(1, min_lane_draws=draws)
            out[name] = c
    yield out
    for name, c in out.items():
        if name != "auto":
            c.close()


@pytest.fixture(scope="module")
def exp(S, oracle):
    """Oracle bytes, computed once per argument set and never modified (callers copy)."""
    @functools.lru_cache(maxsize=None)
    def dgen(size, dedup, compress, seed):
        fn, fd = S.compress_ratio(compress)
        a = oracle.dgen_fill(size, dedup, fn, fd, seed)
        a.setflags(write=False)
        return a

    @functools.lru_cache(maxsize=None)
    def k2(length, chunk, seed_base):
        a = oracle.xoshiro_chunks(length, chunk, seed_base)
        a.setflags(write=False)
        return a

    def stream(size, n, stride, dedup, compress, seed_base, first_obj, fill=0):
        out = np.full((n - 1) * stride + size, fill, np.uint8)
        for j in range(n):
            out[j * stride:j * stride + size] = dgen(size, dedup, compress, S.object_entropy(seed_base, first_obj + j))
        return out

    class E:
        pass
    E.dgen, E.k2, E.stream = staticmethod(dgen), staticmethod(k2), staticmethod(stream)
    return E


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to("cuda:0")


def expect(S, got, want, obj_size=None, stride=None, n=1):
    """The result of verifying `got` against `want`, from numpy: granules are
    4 KiB-aligned within each of the n objects of obj_size bytes at `stride`
    (None: one object = the whole buffer); gaps are not compared."""
    if obj_size is None:
        obj_size, stride = len(want), len(want)
    nbytes = nblocks = 0
    first = None
    for j in range(n):
        lo = j * stride
        bad = np.nonzero(got[lo:lo + obj_size] != want[lo:lo + obj_size])[0]
        if bad.size:
            nbytes += int(bad.size)
            nblocks += int(np.unique(bad // BLK).size)
            first = lo + int(bad[0]) if first is None else first
    return S.VerifyResult() if first is None else S.VerifyResult(nbytes, nblocks, first)


def zlen_of(S, clen, compress):
    fn, fd = S.compress_ratio(compress)
    return clen * fn // fd


# ---- 1. clean objects on every lane path ------------------------------------------

@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("compress", COMPRESS, ids=str)
def test_clean_dgen(S, torch, ctxs, exp, path, compress):
    ctx = ctxs[path]
    for size in DG1_SIZES:
        for dedup in DEDUPS:
            t = dev(torch, exp.dgen(size, dedup, compress, 42))
            r = ctx.verify_dgen(t, size, dedup=dedup, compress=compress, seed=42)
            assert r == S.VerifyResult() and r.ok and r.first_offset is None, (size, dedup, r)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("lo,hi", [(1, 3), (2, None)])
def test_clean_dgen_block_range(S, torch, ctxs, exp, path, lo, hi):
    size, dedup, compress = 3 * MIB + 13, 2, 3
    want = exp.dgen(size, dedup, compress, 9)
    end = size if hi is None else hi * MIB
    t = dev(torch, want[lo * MIB:end])
    kw = dict(blk_lo=lo, blk_hi=hi, dedup=dedup, compress=compress, seed=9)
    assert ctxs[path].verify_dgen(t, size, **kw) == S.VerifyResult()
    p = end - lo * MIB - 1                       # the range's last byte; offsets count from src
    t[p] ^= 0xFF
    assert ctxs[path].verify_dgen(t, size, **kw) == S.VerifyResult(1, 1, p)
    assert ctxs[path].verify_dgen(t, size, blk_lo=2, blk_hi=2, seed=9) == S.VerifyResult()   # empty range


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("chunk", [4096, 32768, 2 * MIB])
def test_clean_k2(S, torch, ctxs, exp, path, chunk):
    ctx = ctxs[path]
    lengths = [t for t in range(1, 8)] + [chunk, 3 * chunk] + [2 * chunk + t for t in range(1, 8)]
    for n in lengths:
        want = exp.k2(n, chunk, 1000)
        t = dev(torch, want)
        assert ctx.verify_xoshiro(t, n, chunk_bytes=chunk, seed_base=1000) == S.VerifyResult(), n
        t[n - 1] ^= 0xFF                         # the tail draw's last byte / the chunk's last byte
        assert ctx.verify_xoshiro(t, n, chunk_bytes=chunk, seed_base=1000) == S.VerifyResult(1, 1, n - 1), n
    with pytest.raises(ValueError, match="multiple of 4096"):
        ctx.verify_xoshiro(dev(torch, np.zeros(256, np.uint8)), 256, chunk_bytes=128)


def test_default_plan_64mib(S, torch, gpu_ctx, exp):
    size = 64 * MIB
    t = dev(torch, exp.dgen(size, 1, 1, 5))
    assert gpu_ctx.verify_dgen(t, size, seed=5) == S.VerifyResult()
    for p in (0, 17 * MIB + 4097, size - 1):
        t[p] ^= 0xFF
    assert gpu_ctx.verify_dgen(t, size, seed=5) == S.VerifyResult(3, 3, 0)
    t2 = dev(torch, exp.dgen(size, 1, 2, 5))
    assert gpu_ctx.verify_dgen(t2, size, compress=2, seed=5) == S.VerifyResult()


# ---- 2. one corrupted byte at each boundary the kernel distinguishes ---------------

def boundary_positions(S, path, size, compress):
    z = zlen_of(S, MIB, compress)                # block 0's zero prefix (a full block)
    region = DG1_REGION[path]
    k = (z + 70000) // region * region + region  # a lane-region edge past the prefix, in block 0
    if k >= MIB:
        k = MIB
    ks = z + 5000                                # keystream bytes of block 0
    pos = {
        "first": 0, "last": size - 1,
        "prefix_last": z - 1, "prefix_next": z,
        "piece_lo": ks // 16 * 16 - 1, "piece_hi": ks // 16 * 16,
        "row_lo": ks // 512 * 512 - 1, "row_hi": ks // 512 * 512,
        "granule_lo": ks // BLK * BLK - 1, "granule_hi": ks // BLK * BLK,
        "region_lo": k - 1, "region_hi": k,
        "block_lo": MIB - 1, "block_hi": MIB, "block2_lo": 2 * MIB - 1, "block2_hi": 2 * MIB,
        "ragged": size - 2,
    }
    for b in range(size & 7):                    # the tail draw's bytes
        pos[f"tail{b}"] = (size & ~7) + b
    return {k_: p for k_, p in pos.items() if 0 <= p < size}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("compress", [1, 3], ids=str)
def test_one_corrupted_byte(S, torch, ctxs, exp, path, compress):
    # 2 MiB + 4100: the last block's tail draw is a 4-byte `>> 32` one, its last piece has 4 bytes
    size, dedup, seed = 2 * MIB + 4100, 1, 77
    ctx = ctxs[path]
    t = dev(torch, exp.dgen(size, dedup, compress, seed))
    kw = dict(dedup=dedup, compress=compress, seed=seed)
    pos = boundary_positions(S, path, size, compress)
    for name, p in pos.items():
        t[p] ^= 0xFF
        r = ctx.verify_dgen(t, size, **kw)
        t[p] ^= 0xFF
        assert r == S.VerifyResult(1, 1, p), (name, p, r)
    assert ctx.verify_dgen(t, size, **kw) == S.VerifyResult()
    allp = sorted(set(pos.values()))
    for p in allp:
        t[p] ^= 0xFF
    r = ctx.verify_dgen(t, size, **kw)
    assert r == S.VerifyResult(len(allp), len({p // BLK for p in allp}), allp[0]), r


@pytest.mark.parametrize("path", list(PATHS))
def test_two_bytes_granule_counts(S, torch, ctxs, exp, path):
    size, seed = 2 * MIB + 4100, 78
    ctx = ctxs[path]
    t = dev(torch, exp.dgen(size, 1, 1, seed))
    region = DG1_REGION[path]
    base = MIB + 3 * region if MIB + 5 * region <= 2 * MIB else MIB     # a lane region's start in block 1
    cases = {
        "one_granule": ((base + 5, base + 4000), 1),
        "two_lanes": ((base + region - 1, base + region), 2) if base + region < size else ((MIB - 1, MIB), 2),
    }
    if region >= 2 * BLK:
        cases["one_lane"] = ((base + BLK - 1, base + BLK), 2)
        cases["one_lane_far"] = ((base + 7, base + BLK + 600), 2)
    for name, (pp, blocks) in cases.items():
        for p in pp:
            t[p] ^= 0xFF
        r = ctx.verify_dgen(t, size, seed=seed)
        for p in pp:
            t[p] ^= 0xFF
        assert r == S.VerifyResult(2, blocks, min(pp)), (name, pp, r)


@pytest.mark.parametrize("path", ["auto", "vec"])
def test_each_bit(S, torch, ctxs, exp, path):
    size, compress, seed = MIB + 13, 3, 3
    ctx = ctxs[path]
    t = dev(torch, exp.dgen(size, 1, compress, seed))
    z = zlen_of(S, MIB, compress)
    for p in (z - 3, z + 1000, size - 1):        # in the zero prefix, in the keystream, in the ragged piece
        for bit in range(8):
            t[p] ^= 1 << bit
            r = ctx.verify_dgen(t, size, compress=compress, seed=seed)
            t[p] ^= 1 << bit
            assert r == S.VerifyResult(1, 1, p), (p, bit, r)
    n, chunk = 32768 + 5, 32768
    t = dev(torch, exp.k2(n, chunk, 4))
    for p in (100, n - 1):
        for bit in range(8):
            t[p] ^= 1 << bit
            r = ctx.verify_xoshiro(t, n, chunk_bytes=chunk, seed_base=4)
            t[p] ^= 1 << bit
            assert r == S.VerifyResult(1, 1, p), (p, bit, r)


# ---- 3. seeded fuzz through the three device calls ---------------------------------

def corrupt(rng, a, edges):
    """Bit flips, overwrites and runs that straddle one of `edges`."""
    n = len(a)
    for _ in range(rng.randint(1, 6)):
        kind = rng.randrange(3)
        if kind == 0:
            a[rng.randrange(n)] ^= 1 << rng.randrange(8)
        elif kind == 1:
            p = rng.randrange(n)
            k = min(n - p, rng.randint(1, 40))
            a[p:p + k] = np.frombuffer(rng.randbytes(k), np.uint8)   # may repeat the byte that was there
        else:
            e = rng.choice(edges)
            lo, hi = max(0, e - rng.randint(1, 30)), min(n, e + rng.randint(1, 30))
            if lo < hi:
                a[lo:hi] ^= 0x5A


@pytest.mark.parametrize("seed", range(4 * SOAK))
def test_fuzz(S, torch, ctxs, exp, seed):
    rng = random.Random(0xD61 + seed)
    ctx = ctxs[rng.choice(list(PATHS))]
    dedup, compress = rng.choice(DEDUPS), rng.choice(COMPRESS)
    # one DG1 object
    size = rng.choice([MIB, 2 * MIB, 3 * MIB]) + rng.choice([0, 0, 3, 13, 4100, -1, -4099])
    want = exp.dgen(size, dedup, compress, 1234 + seed)
    got = np.array(want)
    z = zlen_of(S, MIB, compress)
    corrupt(rng, got, [e for e in (z, MIB, 2 * MIB, size, 65536, z // BLK * BLK + BLK) if 0 < e <= size])
    r = ctx.verify_dgen(dev(torch, got), size, dedup=dedup, compress=compress, seed=1234 + seed)
    assert r == expect(S, got, want), ("dgen", size, dedup, compress, r)
    # a stream of DG1 objects
    osz = MIB + rng.choice([0, 100, 4099, -5])
    n, stride = rng.randint(2, 4), MIB + 2 * BLK
    first = rng.randrange(1000)
    wants = exp.stream(osz, n, stride, dedup, compress, 99 + seed, first, fill=0xEE)
    gots = np.array(wants)
    j = rng.randrange(n)
    corrupt(rng, gots[j * stride:j * stride + osz], [z, osz, osz // 2 // 16 * 16] if z else [osz, osz // 2 // 16 * 16])
    r = ctx.verify_dgen_stream(dev(torch, gots), osz, n, stride, dedup=dedup, compress=compress,
                               seed_base=99 + seed, first_obj=first)
    assert r == expect(S, gots, wants, osz, stride, n), ("stream", osz, n, j, r)
    # K2
    chunk = rng.choice([4096, 32768, 2 * MIB])
    length = chunk * rng.randint(1, 3) + rng.choice([0, 1, 5, 7, 12])
    wantk = exp.k2(length, chunk, 7 + seed)
    gotk = np.array(wantk)
    corrupt(rng, gotk, [chunk, length, length & ~7, 4096])
    r = ctx.verify_xoshiro(dev(torch, gotk), length, chunk_bytes=chunk, seed_base=7 + seed)
    assert r == expect(S, gotk, wantk), ("k2", chunk, length, r)


# ---- 4. wrong parameters ------------------------------------------------------------

def test_wrong_parameters(S, torch, gpu_ctx, exp):
    size = 4 * MIB
    have = exp.dgen(size, 2, 2, 11)
    t = dev(torch, have)
    assert gpu_ctx.verify_dgen(t, size, dedup=2, compress=2, seed=11) == S.VerifyResult()
    for dedup, compress, seed in [(2, 2, 12), (1, 2, 11), (2, 1, 11), (2, 3, 11), (3, (3, 2), 13)]:
        want = expect(S, have, exp.dgen(size, dedup, compress, seed))
        assert not want.ok
        assert gpu_ctx.verify_dgen(t, size, dedup=dedup, compress=compress, seed=seed) == want, (dedup, compress, seed)
    # every granule of every block wrong
    r = gpu_ctx.verify_dgen(dev(torch, exp.dgen(size, 1, 1, 11)), size, seed=12)
    assert r == expect(S, exp.dgen(size, 1, 1, 11), exp.dgen(size, 1, 1, 12))
    assert r.mismatched_blocks == size // BLK and r.first_offset == 0
    # first_obj
    osz, n = MIB + 100, 3
    stride = MIB + BLK
    have = exp.stream(osz, n, stride, 1, 1, 50, 7)
    r = gpu_ctx.verify_dgen_stream(dev(torch, have), osz, n, stride, seed_base=50, first_obj=8)
    assert r == expect(S, have, exp.stream(osz, n, stride, 1, 1, 50, 8), osz, stride, n)
    assert r.mismatched_blocks == n * 257
    # K2 seed
    wantk = expect(S, exp.k2(MIB, 32768, 1), exp.k2(MIB, 32768, 2))
    assert gpu_ctx.verify_xoshiro(dev(torch, exp.k2(MIB, 32768, 1)), MIB, chunk_bytes=32768, seed_base=2) == wantk


# ---- 5. streams -------------------------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "uni"])
def test_stream_gaps(S, torch, ctxs, exp, path):
    osz, n, dedup, compress = MIB + 100, 5, 2, 2
    stride = (osz + BLK - 1) // BLK * BLK
    kw = dict(dedup=dedup, compress=compress, seed_base=31, first_obj=4)
    want = exp.stream(osz, n, stride, dedup, compress, 31, 4, fill=0xC3)     # garbage in the gaps
    t = dev(torch, want)
    assert ctxs[path].verify_dgen_stream(t, osz, n, stride, **kw) == S.VerifyResult()
    p = 3 * stride + MIB + 57                      # object 3's short last block
    q = 3 * stride + 9
    t[p] ^= 0xFF
    assert ctxs[path].verify_dgen_stream(t, osz, n, stride, **kw) == S.VerifyResult(1, 1, p)
    t[q] ^= 0xFF
    assert ctxs[path].verify_dgen_stream(t, osz, n, stride, **kw) == S.VerifyResult(2, 2, q)
    with pytest.raises(ValueError, match="overlap"):
        ctxs[path].verify_dgen_stream(t, osz, 2, osz - 4, **kw)               # overlapping objects


def test_stream_stride_above_4gib(S, torch, gpu_ctx, exp):
    osz = MIB + 100
    stride = (4 << 30) + BLK
    t = torch.empty(stride + osz, dtype=torch.uint8, device="cuda:0")        # the gap stays uninitialised
    for j in range(2):
        t[j * stride:j * stride + osz] = dev(torch, exp.dgen(osz, 1, 1, S.object_entropy(8, j)))
    assert gpu_ctx.verify_dgen_stream(t, osz, 2, stride, seed_base=8) == S.VerifyResult()
    p = stride + MIB + 99
    t[p] ^= 0xFF
    assert gpu_ctx.verify_dgen_stream(t, osz, 2, stride, seed_base=8) == S.VerifyResult(1, 1, p)
    del t
    torch.cuda.empty_cache()


# ---- 6. two threads on two streams ---------------------------------------------------

def test_two_threads_two_streams(S, torch, gpu_ctx, exp):
    size, seed = 2 * MIB + 13, 21
    good = dev(torch, exp.dgen(size, 1, 2, seed))
    bad = good.clone()
    flips = [5, 6, MIB + 4096, 2 * MIB + 12]
    for p in flips:
        bad[p] ^= 0xFF
    bufs = [good, bad]
    want = [S.VerifyResult(), S.VerifyResult(4, 3, 5)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got, errs = [[], []], []

    def work(k):
        try:
            for _ in range(20):
                got[k].append(gpu_ctx.verify_dgen(bufs[k], size, compress=2, seed=seed, stream=streams[k]))
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for k in range(2):
        assert got[k] == [want[k]] * 20


# ---- 7. guards ------------------------------------------------------------------------

@pytest.mark.parametrize("size", [MIB + 100, 4097, 12])
def test_guards(S, torch, gpu_ctx, exp, size):
    """The verify of a ragged object does not depend on what follows it."""
    guard = 8192
    want = exp.dgen(size, 1, 1, 66)
    results = []
    for fill in (0x00, 0xFF):
        t = torch.full((guard + size + guard,), fill, dtype=torch.uint8, device="cuda:0")
        t[guard:guard + size] = dev(torch, want)
        results.append(gpu_ctx.verify_dgen(t[guard:], size, seed=66))
        t[guard + size - 1] ^= 0xFF
        results.append(gpu_ctx.verify_dgen(t[guard:], size, seed=66))
    assert results == [S.VerifyResult(), S.VerifyResult(1, 1, size - 1)] * 2


# ---- 8. the host call -------------------------------------------------------------------

def test_host_call(S, exp):
    size, dedup, compress, seed = 3 * MIB + 13, 2, 3, 1001
    want = exp.dgen(size, dedup, compress, seed)
    a = S.generate_controlled_data_alt(size, dedup, compress, seed)
    assert bytes(a) == want.tobytes()
    assert S.verify_generated_data(a, dedup, compress, seed) == S.VerifyResult()
    g = S.Generator(size, dedup, compress, seed=seed)
    buf = bytearray(size)
    mv, pos = memoryview(buf), 0
    for k in [1, 4095, 70000, MIB + 1, 5, 1 << 30]:    # uneven chunks
        pos += g.fill_chunk(mv[pos:pos + k])
    assert pos == size and g.is_complete()
    assert S.verify_generated_data(buf, dedup, compress, seed) == S.VerifyResult()
    assert S.verify_generated_data(bytes(buf), dedup, compress, seed) == S.VerifyResult()      # read-only
    # unaligned: buf[1:] is the object shifted by one byte, so compare an unaligned copy of the object
    shifted = bytearray(size + 1)
    shifted[1:] = want.tobytes()
    assert S.verify_generated_data(memoryview(shifted)[1:], dedup, compress, seed) == S.VerifyResult()
    shifted[1 + MIB + 7] ^= 0xFF
    assert S.verify_generated_data(memoryview(shifted)[1:], dedup, compress, seed) == S.VerifyResult(1, 1, MIB + 7)
    assert not S.verify_generated_data(buf, dedup, compress, seed + 1).ok


def test_host_call_staging_edge(S, exp):
    size, seed = HOST_CHUNK + MIB + 5, 17
    want = exp.dgen(size, 1, 1, seed)
    assert S.verify_generated_data(want.tobytes(), 1, 1, seed) == S.VerifyResult()
    got = np.array(want)
    flips = [HOST_CHUNK - 1, HOST_CHUNK, size - 1]
    for p in flips:
        one = np.array(want)
        one[p] ^= 0xFF
        assert S.verify_generated_data(one, 1, 1, seed) == S.VerifyResult(1, 1, p), p
        got[p] ^= 0xFF
    assert S.verify_generated_data(got, 1, 1, seed) == S.VerifyResult(3, 3, HOST_CHUNK - 1)
