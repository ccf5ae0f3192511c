"""GPU: payload measurement (k_measure, k_measure_blocks, the distinct count,
k_byte_hist and the surfaces over them).

Every expected number comes from numpy on host bytes, never from a restatement
of the fingerprint: distinct blocks are `len({bytes(b) for b in blocks})` with
the blocks cut per object (a ragged last block is a block of its own), zeros
are `np.count_nonzero(a == 0)`, the histogram is `np.bincount`.  Generated
payloads come from the C oracle (oracle/oracle_c.py).  Every assertion is exact.
"""
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLK = 4096
MiB = 1 << 20
SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 8292, 3 * 4096 + 2080, 64 * 4096, 64 * 4096 + 100, 3 * MiB + 4097]
DEDUPS = [0, 1, 2, 3, 7]
COMPRESS = [1, 2, 3, (3, 2), 128]
HOST_CHUNK = 64 << 20          # the host path's staging chunk


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
def wave_ctx(S, gpu_ctx):
    ctxs = {w: S.Context(0, base_seed=S.DEFAULT_BASE_SEED, waves_per_block=w) for w in (1, 2, 4)}
    yield ctxs
    for c in ctxs.values():
        c.close()


def expect(S, objs, block_bytes, hist=False):
    """The result of measuring the objects (host arrays), from numpy."""
    seen, blocks, nbytes, zeros = set(), 0, 0, 0
    h = np.zeros(256, np.int64)
    for a in objs:
        a = np.ascontiguousarray(a, np.uint8)
        mv = memoryview(a)
        for o in range(0, a.size, block_bytes):
            seen.add(bytes(mv[o:o + block_bytes]))
            blocks += 1
        nbytes += a.size
        zeros += int(np.count_nonzero(a == 0))
        if hist:
            h += np.bincount(a, minlength=256)
    return S.MeasureResult(nbytes, zeros, blocks, len(seen), tuple(int(v) for v in h) if hist else None)


def np_entropy(h):
    h = np.asarray(h, np.float64)
    p = h[h > 0] / h.sum()
    return float(-(p * np.log2(p)).sum())


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to("cuda:0")


@pytest.fixture(scope="module")
def exp(S, oracle, base):
    """Oracle bytes and their expected results, computed once per argument set."""
    class E:
        @staticmethod
        @functools.lru_cache(maxsize=None)
        def controlled(size, dedup, compress, entropy=42):
            fn, fd = S.compress_ratio(compress)
            a = oracle.fill_controlled(size, dedup, fn, fd, entropy, base)
            a.setflags(write=False)
            return a

        @staticmethod
        @functools.lru_cache(maxsize=None)
        def dgen(size, dedup, compress, seed=7):
            fn, fd = S.compress_ratio(compress)
            a = oracle.dgen_fill(size, dedup, fn, fd, seed)
            a.setflags(write=False)
            return a

        @staticmethod
        @functools.lru_cache(maxsize=None)
        def controlled_result(size, dedup, compress, block_bytes):
            return expect(S, [E.controlled(size, dedup, compress)], block_bytes)

        @staticmethod
        @functools.lru_cache(maxsize=None)
        def dgen_result(size, dedup, compress, block_bytes):
            return expect(S, [E.dgen(size, dedup, compress)], block_bytes)
    return E


@pytest.fixture(scope="module")
def dgen_dev(torch, exp):
    """The DG1 payloads of section 2 on the device, uploaded once."""
    @functools.lru_cache(maxsize=None)
    def get(size, dedup, compress):
        return dev(torch, exp.dgen(size, dedup, compress))
    return get


# ---- 1. generated payloads at 4 KiB blocks ----------------------------------------

@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("compress", COMPRESS, ids=str)
def test_controlled_4k(S, torch, wave_ctx, exp, waves, compress):
    ctx = wave_ctx[waves]
    for size in SIZES:
        for dedup in DEDUPS:
            t = dev(torch, exp.controlled(size, dedup, compress))
            got = ctx.measure(t, block_bytes=BLK)
            assert got == exp.controlled_result(size, dedup, compress, BLK), (size, dedup)
            if size % BLK == 0:   # the generator's closed form; a ragged tail is one block more
                assert got.unique_blocks == S.unique_blocks(size // BLK, dedup), (size, dedup)


# ---- 2. DG1 -------------------------------------------------------------------------

@pytest.mark.parametrize("size,dedup,compress,block_bytes,unique,blocks", [
    (8 * MiB, 2, 1, MiB, 4, 8),
    (8 * MiB, 3, 2, MiB, 3, 8),
    (8 * MiB, 3, 2, BLK, 385, 2048),
    (8 * MiB + 5, 2, 2, MiB, 6, 9),      # the closed form gives 5; the 5-byte tail is the sixth
    (64 * MiB, 2, 1, MiB, 32, 64),       # the reference's test_data_dedup_compress1
    (64 * MiB, 2, 1, BLK, 8192, 16384),
    (8 * MiB, 3, 2, 8192, None, 1024),
    (8 * MiB, 3, 2, 65536, None, 128),
    (8 * MiB + 5, 2, 2, 8192, None, 1025),
    (8 * MiB + 5, 2, 2, 65536, None, 129),
    (64 * MiB, 2, 1, 65536, None, 1024),
])
def test_dgen(S, gpu_ctx, exp, dgen_dev, size, dedup, compress, block_bytes, unique, blocks):
    got = gpu_ctx.measure(dgen_dev(size, dedup, compress), block_bytes=block_bytes)
    assert got == exp.dgen_result(size, dedup, compress, block_bytes)
    assert got.blocks == blocks
    if unique is not None:
        assert got.unique_blocks == unique


def test_dgen_zero_fraction(S, torch, gpu_ctx, exp, dgen_dev):
    """The reference tests' own tolerance: |z - (c-1)/c| < 0.05."""
    r1 = gpu_ctx.measure(dgen_dev(64 * MiB, 2, 1), block_bytes=MiB)
    assert r1.zero_bytes == exp.dgen_result(64 * MiB, 2, 1, MiB).zero_bytes
    assert abs(r1.zero_fraction - 0.0) < 0.05
    r2 = gpu_ctx.measure(dev(torch, exp.dgen(16 * MiB, 1, 2)), block_bytes=MiB)
    assert r2 == exp.dgen_result(16 * MiB, 1, 2, MiB)
    assert abs(r2.zero_fraction - 0.5) < 0.05


# ---- 3. crafted blocks ---------------------------------------------------------------

def variants(a):
    """(name, block) pairs: copies of block `a` changed in one small way inside its first 4 KiB."""
    out = []

    def var(name, f):
        b = a.copy()
        f(b)
        assert not np.array_equal(a, b), name
        out.append((name, b))

    for off in (0, 15, 16, 2047, 2048, 4095):
        for bit in range(8):
            def flip(b, off=off, bit=bit):
                b[off] ^= 1 << bit
            var(f"bit{bit}@{off}", flip)

    def swap(b, i, j, w):
        x = b[i:i + w].copy()
        b[i:i + w] = b[j:j + w]
        b[j:j + w] = x
    for p, q in ((0, 1), (0, 64), (3, 255)):
        var(f"pieces{p},{q}", lambda b, p=p, q=q: swap(b, 16 * p, 16 * q, 16))

    def rotate(b):
        b[:4096] = np.roll(b[:4096], 16)
    var("rotate", rotate)
    var("dwords", lambda b: swap(b, 16 * 5 + 0, 16 * 5 + 8, 4))
    var("adjacent dwords", lambda b: swap(b, 16 * 9 + 4, 16 * 9 + 8, 4))
    var("halves", lambda b: swap(b, 16 * 7, 16 * 7 + 8, 8))
    var("bytes", lambda b: swap(b, 16 * 11 + 4, 16 * 11 + 6, 1))

    def move(b, p, q, k):
        b[16 * p + k] += 1
        b[16 * q + k] -= 1
    for p, q, k in ((2, 3, 0), (2, 66, 5), (10, 200, 15)):
        var(f"move{p},{q},{k}", lambda b, p=p, q=q, k=k: move(b, p, q, k))
    return out


@pytest.mark.parametrize("block_bytes", [4096, 8192])
def test_crafted_pairs(S, torch, gpu_ctx, block_bytes):
    rng = np.random.default_rng(1234 + block_bytes)
    a = rng.integers(0, 256, block_bytes, dtype=np.uint8)
    for p, q, k in ((2, 3, 0), (2, 66, 5), (10, 200, 15)):   # room for the +1 / -1 of "move"
        a[16 * p + k] = 100
        a[16 * q + k] = 100
    r = gpu_ctx.measure(dev(torch, np.concatenate([a, a])), block_bytes=block_bytes)
    assert (r.blocks, r.unique_blocks) == (2, 1)
    for name, b in variants(a):
        both = np.concatenate([a, b])
        r = gpu_ctx.measure(dev(torch, both), block_bytes=block_bytes)
        assert r == expect(S, [both], block_bytes), name
        assert (r.blocks, r.unique_blocks) == (2, 2), name
    # all variants and the original at once
    alls = np.concatenate([a] + [b for _, b in variants(a)] + [a])
    r = gpu_ctx.measure(dev(torch, alls), block_bytes=block_bytes)
    assert r == expect(S, [alls], block_bytes)
    assert r.unique_blocks == r.blocks - 1


@pytest.mark.parametrize("block_bytes", [8192, MiB])
def test_granule_order(S, torch, gpu_ctx, block_bytes):
    rng = np.random.default_rng(99)
    a = rng.integers(0, 256, block_bytes, dtype=np.uint8)
    g = a.reshape(-1, BLK)
    swapped = g.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    rolled = np.roll(g, 1, axis=0)
    for name, b in (("swapped", swapped.reshape(-1)), ("rolled", rolled.reshape(-1))):
        both = np.concatenate([a, b])
        r = gpu_ctx.measure(dev(torch, both), block_bytes=block_bytes)
        assert r == expect(S, [both], block_bytes), name
        assert (r.blocks, r.unique_blocks) == (2, 2), name
    same = np.concatenate([a, a, a])
    r = gpu_ctx.measure(dev(torch, same), block_bytes=block_bytes)
    assert (r.blocks, r.unique_blocks) == (3, 1)


@pytest.mark.parametrize("block_bytes", [4096, 8192, 65536])
def test_constant_blocks(S, torch, gpu_ctx, block_bytes):
    n = 64 * 1024
    z, f = np.zeros(n, np.uint8), np.full(n, 0xFF, np.uint8)
    r = gpu_ctx.measure(dev(torch, z), block_bytes=block_bytes)
    assert r == expect(S, [z], block_bytes) and r.unique_blocks == 1 and r.zero_bytes == n
    r = gpu_ctx.measure(dev(torch, f), block_bytes=block_bytes)
    assert r == expect(S, [f], block_bytes) and r.unique_blocks == 1 and r.zero_bytes == 0
    zf = np.concatenate([z, f])
    r = gpu_ctx.measure(dev(torch, zf), block_bytes=block_bytes)
    assert r == expect(S, [zf], block_bytes) and r.unique_blocks == 2 and r.zero_bytes == n


# ---- 4. ragged tails and streams ---------------------------------------------------------

def strided(objs, stride, poison):
    """The objects at a stride, every gap (the one after the last object too) filled with poison."""
    buf = np.empty(stride * len(objs), np.uint8)
    for j, a in enumerate(objs):
        buf[j * stride:j * stride + a.size] = a
        buf[j * stride + a.size:(j + 1) * stride] = (poison + 37 * j) & 0xFF
    return buf


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("block_bytes", [4096, 8192])
def test_ragged_stream_ignores_gaps(S, torch, wave_ctx, block_bytes, waves):
    ctx = wave_ctx[waves]
    rng = np.random.default_rng(5)
    size, stride = 12288 + 100, 12288 + 100 + 4096 + 12   # a 16-byte aligned stride with a > 4 KiB gap
    objs = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(5)]
    objs[3][:8192] = objs[1][:8192]      # shared blocks between objects
    objs[4][-100:] = objs[0][-100:]      # at 4096: a shared 100-byte tail
    want = expect(S, objs, block_bytes)
    got = [ctx.measure_stream(dev(torch, strided(objs, stride, p)), size, 5, stride, block_bytes=block_bytes)
           for p in (0x00, 0xA5)]
    assert got[0] == want and got[1] == want
    assert want.bytes == 5 * size


def test_tails(S, torch, gpu_ctx):
    rng = np.random.default_rng(6)
    tail = rng.integers(0, 256, 100, dtype=np.uint8)
    objs = [np.concatenate([rng.integers(0, 256, BLK, dtype=np.uint8), tail]) for _ in range(4)]
    stride = BLK + 112
    r = gpu_ctx.measure_stream(dev(torch, strided(objs, stride, 0x11)), BLK + 100, 4, stride)
    assert r == expect(S, objs, BLK) and (r.blocks, r.unique_blocks) == (8, 5)   # identical tails count once
    a = rng.integers(0, 256, BLK, dtype=np.uint8)
    one = np.concatenate([a, a[:100]])     # a tail equal to the start of a full block is still its own block
    r = gpu_ctx.measure(dev(torch, one))
    assert r == expect(S, [one], BLK) and (r.blocks, r.unique_blocks) == (2, 2)
    z = np.zeros(BLK + 100, np.uint8)      # the same with zeros: padding must not make them equal
    r = gpu_ctx.measure(dev(torch, z))
    assert r == expect(S, [z], BLK) and (r.blocks, r.unique_blocks) == (2, 2)
    for v in (0, 7):
        b = np.full(1, v, np.uint8)
        r = gpu_ctx.measure(dev(torch, np.concatenate([b, np.full(15, 0xEE, np.uint8)])), nbytes=1)
        assert r == expect(S, [b], BLK) and (r.bytes, r.blocks, r.unique_blocks, r.zero_bytes) == (1, 1, 1, int(v == 0))


def test_stream_across_object_split(S, torch, gpu_ctx):
    """More than 65 535 objects: the launch is split along the objects."""
    n = 65535 + 3
    rng = np.random.default_rng(8)
    table = rng.integers(0, 256, (1000, BLK), dtype=np.uint8)
    table[17, :2048] = 0
    idx = np.arange(n) % 1000
    idx[-3:] = (998, 1, 998)
    buf = table[idx].reshape(-1)
    r = gpu_ctx.measure_stream(dev(torch, buf), BLK, n)
    assert r == expect(S, list(buf.reshape(n, BLK)), BLK)
    assert (r.blocks, r.unique_blocks) == (n, 1000)


def test_object_across_granule_split(S, torch, gpu_ctx):
    """One object of more than 2^22 granules (16 GiB): the launch is split along the granules.
    A zeroed device buffer with three marker bytes; the expected numbers follow from where they
    are (no host copy of 16 GiB): 1 MiB blocks 5 and 16384 carry the same byte at the same
    offset, so they are one block, and block 16384 starts the second sub-launch."""
    n = (16384 + 1) * MiB + 100
    t = torch.zeros(n + 12, dtype=torch.uint8, device="cuda:0")
    for pos in (5 * MiB + 100, 16384 * MiB + 100, 100 * MiB + 3 * BLK + 100):
        t[pos] = 7
    r = gpu_ctx.measure(t, nbytes=n, block_bytes=MiB, hist=True)
    hist = [0] * 256
    hist[0], hist[7] = n - 3, 3
    assert r == S.MeasureResult(n, n - 3, 16386, 4, tuple(hist))   # zeros, two marker blocks, the 100-byte tail
    r = gpu_ctx.measure(t, nbytes=n, block_bytes=BLK)
    assert (r.bytes, r.zero_bytes, r.blocks, r.unique_blocks) == (n, n - 3, 16385 * 256 + 1, 3)
    del t
    torch.cuda.empty_cache()


# ---- 5. accumulation ------------------------------------------------------------------------

def test_adds_reuse_one_buffer(S, torch, gpu_ctx, oracle, base):
    """Three adds over one device buffer that fills on the same stream overwrite, no sync between."""
    size, n, stride = 8292, 4, 8304
    fn, fd = S.compress_ratio(2)
    seeds = (1000, 2000, 3000)
    host = [oracle.fill_stream(size, n, 2, fn, fd, sb, 0, base, stride=stride) for sb in seeds]
    objs = [h[j * stride:j * stride + size] for h in host for j in range(n)]
    t = torch.zeros(stride * n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with gpu_ctx.measurer(BLK) as m:
        for sb in seeds:
            gpu_ctx.fill_stream(t, size, n, stride, dedup=2, compress=2, seed_base=sb, stream=st)
            m.add_stream(t, size, n, stride, stream=st)
        r = m.result()
        assert r == expect(S, objs, BLK)
        # the same seeds again: twice the blocks, nothing new
        for sb in seeds:
            gpu_ctx.fill_stream(t, size, n, stride, dedup=2, compress=2, seed_base=sb, stream=st)
            m.add_stream(t, size, n, stride, stream=st)
        r2 = m.result()
        assert (r2.blocks, r2.bytes, r2.zero_bytes) == (2 * r.blocks, 2 * r.bytes, 2 * r.zero_bytes)
        assert r2.unique_blocks == r.unique_blocks
    one = gpu_ctx.measure_stream(dev(torch, np.concatenate([strided([o], stride, 0) for o in objs])), size, 3 * n,
                                 stride)
    assert one == r
    st.synchronize()


@pytest.mark.parametrize("block_bytes", [4096, 65536])
def test_ranges_equal_the_whole(S, torch, gpu_ctx, exp, block_bytes):
    size = 3 * MiB + 4097
    a = exp.controlled(size, 3, 2)
    t = dev(torch, a)
    nb = -(-size // block_bytes)
    cuts = [0, nb // 7, nb // 7 + 1, nb // 2, nb + 5]
    with gpu_ctx.measurer(block_bytes) as m:
        for lo, hi in zip(cuts, cuts[1:]):
            m.add_range(t[lo * block_bytes:], size, lo, hi)
        m.add_range(t, size, 3, 3)             # empty ranges add nothing
        m.add_range(t, size, nb, nb + 1)
        r = m.result()
    assert r == expect(S, [a], block_bytes) == gpu_ctx.measure(t, block_bytes=block_bytes)


def test_two_streams_two_threads(S, torch, gpu_ctx, exp):
    parts = [exp.controlled(64 * 4096 + 100, 2, 2), exp.controlled(3 * MiB + 4097, 3, 1)]
    ts = [dev(torch, p) for p in parts]
    torch.cuda.synchronize()               # the uploads ran on the default stream
    errs = []
    with gpu_ctx.measurer(BLK) as m:
        def work(k):
            try:
                st = torch.cuda.Stream()
                for _ in range(4):
                    m.add(ts[k], stream=st)
            except Exception as e:   # pragma: no cover
                errs.append(e)
        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs
        r = m.result()
    want = expect(S, parts, BLK)
    assert (r.bytes, r.zero_bytes, r.blocks) == (4 * want.bytes, 4 * want.zero_bytes, 4 * want.blocks)
    assert r.unique_blocks == want.unique_blocks


def test_result_is_not_destructive(S, torch, gpu_ctx, exp):
    a, b = exp.controlled(64 * 4096, 2, 2), exp.controlled(8292, 1, 1)
    with gpu_ctx.measurer(BLK, hist=True) as m:
        assert m.result() == S.MeasureResult(hist=(0,) * 256)
        m.add(dev(torch, a))
        r1 = m.result()
        assert r1 == m.result() == expect(S, [a], BLK, hist=True)
        m.add(dev(torch, b))
        assert m.result() == expect(S, [a, b], BLK, hist=True)
        m.reset()
        assert m.result() == S.MeasureResult(hist=(0,) * 256)
        m.add(dev(torch, b))
        assert m.result() == expect(S, [b], BLK, hist=True)
    with gpu_ctx.measurer(BLK) as m:
        m.add_stream(0, 0, 5)                  # zero-length adds launch nothing, whatever the pointer
        m.add_stream(0, 4096, 0)
        assert m.result() == S.MeasureResult()


def test_array_growth(S, torch, gpu_ctx, oracle, base):
    """65 536 fingerprints added in uneven pieces: the array doubles several times."""
    size = 256 * MiB
    a = oracle.fill_stream(size, 1, 4, 0, 1, 77, 0, base, threads=8)
    t = dev(torch, a)
    nb = size // BLK
    cuts = [0, 1, 1000, 5000, 5001, 30000, nb]
    with gpu_ctx.measurer(BLK) as m:
        for lo, hi in zip(cuts, cuts[1:]):
            m.add_range(t[lo * BLK:], size, lo, hi)
        r = m.result()
    assert r == expect(S, [a], BLK)
    assert (r.blocks, r.unique_blocks) == (nb, S.unique_blocks(nb, 4))


# ---- 6. histogram ----------------------------------------------------------------------------

def test_histogram(S, torch, gpu_ctx, exp):
    rng = np.random.default_rng(3)
    cases = [exp.controlled(64 * 4096 + 100, 1, 1), exp.controlled(64 * 4096 + 100, 2, 3), exp.dgen(8 * MiB, 2, 1),
             np.zeros(65536, np.uint8), np.full(65536, 0xFF, np.uint8), np.full(1, 9, np.uint8),
             np.zeros(1, np.uint8), rng.integers(0, 4, 100001, dtype=np.uint8)]
    for a in cases:
        pad = np.concatenate([a, np.full(-a.size % 16, 0xEE, np.uint8)])
        r = gpu_ctx.measure(dev(torch, pad), nbytes=a.size, hist=True)
        assert r == expect(S, [a], BLK, hist=True), a.size
        assert r.hist == tuple(int(v) for v in np.bincount(a, minlength=256))
        assert abs(r.entropy_bits - np_entropy(r.hist)) <= 1e-12
        plain = gpu_ctx.measure(dev(torch, pad), nbytes=a.size)
        assert plain.hist is None and plain.entropy_bits is None and plain.zero_bytes == r.zero_bytes


def test_histogram_ragged_stream(S, torch, gpu_ctx):
    rng = np.random.default_rng(4)
    size, stride = 12288 + 100, 12288 + 100 + 4096 + 12
    objs = [rng.integers(0, 7, size, dtype=np.uint8) for _ in range(5)]
    want = expect(S, objs, BLK, hist=True)
    for p in (0x00, 0x03):
        assert gpu_ctx.measure_stream(dev(torch, strided(objs, stride, p)), size, 5, stride, hist=True) == want


# ---- 7. host buffers ---------------------------------------------------------------------------

def test_measure_data_buffers(S, exp):
    a = exp.controlled(64 * 4096 + 100, 2, 2)
    want = expect(S, [a], BLK, hist=True)
    assert S.measure_data(bytearray(a.tobytes()), hist=True) == want
    assert S.measure_data(a.tobytes(), hist=True) == want                  # read-only bytes
    shifted = np.empty(a.size + 1, np.uint8)
    shifted[1:] = a
    assert S.measure_data(shifted[1:], hist=True) == want                  # a view at offset 1
    assert S.measure_data(a) == expect(S, [a], BLK)
    assert S.measure_data(b"") == S.MeasureResult()


@pytest.mark.parametrize("block_bytes", [4096, MiB])
def test_measure_data_across_the_chunk_edge(S, exp, block_bytes):
    a = exp.dgen(HOST_CHUNK + 4097, 2, 2)
    assert S.measure_data(a, block_bytes=block_bytes) == expect(S, [a], block_bytes)


# ---- 8. refusals on the device ---------------------------------------------------------------------

def test_refusals(S, torch, gpu_ctx):
    t = torch.zeros(3 * 8192, dtype=torch.uint8, device="cuda:0")
    with gpu_ctx.measurer(BLK) as m:
        with pytest.raises(ValueError, match="16-byte aligned"):
            m.add_stream(t[8:], 4096, 2, 4096)
        with pytest.raises(ValueError, match="16-byte aligned"):
            m.add_stream(t, 4096, 2, 4104)
        with pytest.raises(ValueError, match="overlap"):
            m.add_stream(t, 8192, 2, 4096)
        with pytest.raises(ValueError, match="16-byte aligned"):
            m.add_range(t[4:], 8192, 0, 1)
        with pytest.raises(ValueError, match="holds"):
            m.add_stream(t, 8192, 4)
        assert m.result() == S.MeasureResult()
    for bb in (0, 4095, 6000, 2**31):
        with pytest.raises(ValueError, match="block_bytes"):
            gpu_ctx.measurer(bb)


# ---- 9. block sizes that are no power of two -----------------------------------------------------
# gpb = 3, 5, 15 (the last one-thread-per-block size), 17 (the first odd one-wave-per-block size)
# and 65 (that kernel's second lap).

ODD_BB = [12288, 20480, 61440, 69632, 266240]
TABLE_SEQ = [0, 1, 2, 1, 0, 3, 3, 4, 5, 6, 2]
TABLE_K = 7
TABLE_TAIL = 4096 + 100


@functools.lru_cache(maxsize=None)
def table_objects(block_bytes):
    """Five objects over one table of K random blocks (the first half of block 3 zeroed, block 6
    equal to block 5 up to its last byte): object j is the blocks TABLE_SEQ rotated by j, then a
    ragged tail equal to the start of block 1."""
    rng = np.random.default_rng(4000 + block_bytes)
    table = rng.integers(0, 256, (TABLE_K, block_bytes), dtype=np.uint8)
    table[3, :block_bytes // 2] = 0
    table[6] = table[5]
    table[6, -1] ^= 0x80
    assert len({bytes(b) for b in table}) == TABLE_K
    objs = []
    for j in range(5):
        a = np.concatenate([table[np.roll(TABLE_SEQ, -j)].reshape(-1), table[1, :TABLE_TAIL]])
        a.setflags(write=False)
        objs.append(a)
    return objs


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("block_bytes", ODD_BB)
def test_odd_block_tables(S, torch, wave_ctx, block_bytes, waves):
    ctx = wave_ctx[waves]
    objs = table_objects(block_bytes)
    one, size, nb = objs[0], objs[0].size, len(TABLE_SEQ) + 1
    assert size == len(TABLE_SEQ) * block_bytes + TABLE_TAIL
    want = expect(S, [one], block_bytes)
    # the closed form first: every table block occurs, the tail is a block of its own
    assert (want.bytes, want.blocks, want.unique_blocks) == (size, nb, TABLE_K + 1)
    t = dev(torch, one)
    whole = ctx.measure(t, block_bytes=block_bytes)
    assert whole == want
    cuts = [0, 1, 2, nb // 2, nb + 5]
    with ctx.measurer(block_bytes) as m:
        for lo, hi in zip(cuts, cuts[1:]):
            m.add_range(t[lo * block_bytes:], size, lo, hi)
        m.add_range(t, size, 3, 3)             # empty ranges add nothing
        m.add_range(t, size, nb, nb + 1)
        assert m.result() == want
    with ctx.measurer(block_bytes) as m:      # the object twice in one handle
        m.add(t)
        m.add(t)
        r2 = m.result()
    assert (r2.bytes, r2.zero_bytes, r2.blocks) == (2 * want.bytes, 2 * want.zero_bytes, 2 * want.blocks)
    assert r2.unique_blocks == want.unique_blocks
    # five objects, the sequence rotated from one to the next: the same blocks at other places
    stride = -(-(size + 4096 + 12) // 16) * 16
    wants = expect(S, objs, block_bytes)
    assert (wants.bytes, wants.blocks, wants.unique_blocks) == (5 * size, 5 * nb, TABLE_K + 1)
    assert wants.zero_bytes == 5 * want.zero_bytes
    for p in (0x00, 0xA5):
        got = ctx.measure_stream(dev(torch, strided(objs, stride, p)), size, 5, stride, block_bytes=block_bytes)
        assert got == wants, hex(p)


@pytest.mark.parametrize("block_bytes", ODD_BB)
def test_odd_block_generated(S, torch, gpu_ctx, exp, dgen_dev, block_bytes):
    a = exp.dgen(8 * MiB + 5, 2, 2)
    want = expect(S, [a], block_bytes, hist=True)
    assert want.blocks == -(-a.size // block_bytes)
    assert gpu_ctx.measure(dgen_dev(8 * MiB + 5, 2, 2), block_bytes=block_bytes, hist=True) == want
    b = exp.controlled(3 * MiB + 4097, 3, 2)
    want = expect(S, [b], block_bytes)
    assert want.blocks == -(-b.size // block_bytes)
    assert gpu_ctx.measure(dev(torch, b), block_bytes=block_bytes) == want


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("block_bytes", [12288, 69632])
def test_odd_block_edge_sizes(S, torch, wave_ctx, block_bytes, waves):
    ctx = wave_ctx[waves]
    bb = block_bytes
    rng = np.random.default_rng(4100 + bb)
    for size in (1, bb - 16, bb - 1, bb, bb + 1, bb + 4096, 2 * bb + 4097, 3 * bb + 2080):
        a = rng.integers(0, 256, size, dtype=np.uint8)
        want = expect(S, [a], bb)
        assert (want.bytes, want.blocks, want.unique_blocks) == (size, -(-size // bb), -(-size // bb)), size
        assert ctx.measure(dev(torch, a), block_bytes=bb) == want, size


@functools.lru_cache(maxsize=None)
def switch_objects(block_bytes):
    """Five objects of two full blocks and a ragged third of 4096 + 5 bytes: random, but for
    a block shared by two objects, a run of zeros and two equal ragged blocks."""
    rng = np.random.default_rng(4200 + block_bytes)
    objs = [rng.integers(0, 256, 2 * block_bytes + 4096 + 5, dtype=np.uint8) for _ in range(5)]
    objs[1][:block_bytes] = objs[0][:block_bytes]
    objs[2][block_bytes + 100:block_bytes + 5100] = 0
    objs[4][2 * block_bytes:] = objs[3][2 * block_bytes:]
    for a in objs:
        a.setflags(write=False)
    return objs


@pytest.mark.parametrize("form", ["stream", "batch"])
@pytest.mark.parametrize("block_bytes", [15 * 4096, 16 * 4096])
def test_pass2_at_the_thread_wave_switch(S, torch, gpu_ctx, block_bytes, form):
    """Blocks of 15 granules (the last size summed by one thread) and of 16 (the first summed by
    one wave), through add_stream and add_batch: 15 blocks, so the wave form's last workgroup of
    four holds three."""
    objs = switch_objects(block_bytes)
    size = objs[0].size
    stride = -(-(size + 4096 + 12) // 16) * 16
    want = expect(S, objs, block_bytes, hist=True)
    assert (want.bytes, want.blocks, want.unique_blocks) == (5 * size, 15, 13)
    assert want.zero_bytes >= 5000
    t = dev(torch, strided(objs, stride, 0xA5))
    with gpu_ctx.measurer(block_bytes, hist=True) as m:
        if form == "stream":
            m.add_stream(t, size, 5, stride)
        else:
            m.add_batch(t, [(j * stride, size) for j in range(5)])
        assert m.result() == want


# ---- 10. every piece enters the fingerprint, under a key of its own ---------------------------------

def piece_set(block_bytes):
    """The pieces that get a variant: all of a small block, granules 0, 8 and 16 of a 17-granule one."""
    if block_bytes <= 12288:
        return list(range(block_bytes // 16))
    return [256 * g + k for g in (0, 8, 16) for k in range(256)]


def distinct_piece_block(block_bytes, seed):
    """A random block with no two equal 16-byte pieces, so that no exchange of two is a no-op."""
    P = block_bytes // 16
    while True:
        a = np.random.default_rng(seed).integers(0, 256, block_bytes, dtype=np.uint8)
        if len({bytes(x) for x in a.reshape(P, 16)}) == P:
            return a
        seed += 1


def flipped(a, pieces):
    """One copy of `a` per piece p, bit p % 128 of that piece flipped."""
    out = np.tile(a, (len(pieces), 1))
    for i, p in enumerate(pieces):
        bit = p % 128
        out[i, 16 * p + bit // 8] ^= 1 << (bit % 8)
    return out


def swapped(a, pieces):
    """One copy of `a` per piece p and index bit b clear in p with q = p | 1 << b inside the block,
    pieces p and q exchanged: any two pieces whose indices differ in one bit."""
    P = a.size // 16
    pairs = [(p, p | (1 << b)) for p in pieces for b in range(P.bit_length())
             if not p >> b & 1 and p | (1 << b) < P]
    out = np.tile(a, (len(pairs), 1))
    for i, (p, q) in enumerate(pairs):
        out[i, 16 * p:16 * p + 16] = a[16 * q:16 * q + 16]
        out[i, 16 * q:16 * q + 16] = a[16 * p:16 * p + 16]
    return out


@functools.lru_cache(maxsize=None)
def piece_case(S, block_bytes):
    """[a] + the flips + the swaps + [a] as one buffer, with its expected result, built once and
    shared by the wave counts: 256 + 1024 variants (5.3 MB) at 4096, 768 + 3584 (53.5 MB) at 12288,
    768 + 5120 (410 MB) at 69632."""
    a = distinct_piece_block(block_bytes, 5000 + block_bytes)
    P = block_bytes // 16
    assert len({bytes(x) for x in a.reshape(P, 16)}) == P
    pieces = piece_set(block_bytes)
    buf = np.concatenate([a[None], flipped(a, pieces), swapped(a, pieces), a[None]]).reshape(-1)
    buf.setflags(write=False)
    return buf, expect(S, [buf], block_bytes)


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("block_bytes", [4096, 12288, 69632])
def test_every_piece_and_key(S, torch, wave_ctx, block_bytes, waves):
    buf, want = piece_case(S, block_bytes)
    assert want.blocks == buf.size // block_bytes > 2 * len(piece_set(block_bytes))
    assert want.unique_blocks == want.blocks - 1      # numpy: every variant differs from `a` and from the others
    t = dev(torch, buf)
    got = wave_ctx[waves].measure(t, block_bytes=block_bytes)
    del t
    assert got == want


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_every_piece_stream(S, torch, wave_ctx, waves):
    """The flips at 12288 as objects of their own, each with the same 100-byte tail."""
    bb = 12288
    a = distinct_piece_block(bb, 5000 + bb)
    rng = np.random.default_rng(5100)
    tail = rng.integers(0, 256, 100, dtype=np.uint8)
    blocks = np.concatenate([a[None], flipped(a, piece_set(bb)), a[None]])
    objs = [np.concatenate([b, tail]) for b in blocks]
    size, stride = bb + 100, bb + 112
    want = expect(S, objs, bb)
    assert (want.blocks, want.unique_blocks) == (2 * len(objs), bb // 16 + 1 + 1)   # the flips, `a`, the tail
    got = wave_ctx[waves].measure_stream(dev(torch, strided(objs, stride, 0xA5)), size, len(objs), stride,
                                         block_bytes=bb)
    assert got == want


# ---- 11. the largest blocks ----------------------------------------------------------------------------
# Zeroed device buffers with marker bytes, as in test_object_across_granule_split: the expected
# numbers follow from where the markers are.

def test_block_of_one_gib(S, torch, gpu_ctx):
    """block_bytes = 2^30: gpb = 262144, piece indices up to 2^26, 4096 laps per lane in pass 2."""
    bb = 1 << 30
    n = 2 * bb + 100
    t = torch.zeros(n + 12, dtype=torch.uint8, device="cuda:0")
    t[bb - 1] = 7
    t[2 * bb - 1] = 7
    hist = [0] * 256
    hist[0], hist[7] = n - 2, 2
    r = gpu_ctx.measure(t, nbytes=n, block_bytes=bb, hist=True)
    assert r == S.MeasureResult(n, n - 2, 3, 2, tuple(hist))     # two equal blocks and the 100-byte tail
    t[2 * bb - 1] = 0
    t[2 * bb - 2] = 7                                            # the last piece of block 1, one byte down
    r = gpu_ctx.measure(t, nbytes=n, block_bytes=bb, hist=True)
    assert r == S.MeasureResult(n, n - 2, 3, 3, tuple(hist))
    del t
    torch.cuda.empty_cache()


def test_block_of_one_gib_less_a_granule(S, torch, gpu_ctx):
    """block_bytes = 2^30 - 4096: gpb = 262143, odd, on the one-wave-per-block kernel."""
    bb = (1 << 30) - 4096
    n = 1 << 31
    t = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    t[bb - 1] = 7
    t[2 * bb - 1] = 7
    r = gpu_ctx.measure(t, nbytes=n, block_bytes=bb)
    assert n - 2 * bb == 8192
    assert r == S.MeasureResult(n, n - 2, 3, 2)                  # two equal blocks and 8192 zeros
    t[2 * bb - 1] = 0
    t[2 * bb - 4097] = 7                                         # the same byte one granule down
    r = gpu_ctx.measure(t, nbytes=n, block_bytes=bb)
    assert r == S.MeasureResult(n, n - 2, 3, 3)
    del t
    torch.cuda.empty_cache()


# ---- 12. host buffers across the chunking ----------------------------------------------------------------

@pytest.mark.parametrize("hist", [False, True])
def test_measure_data_chunk_of_odd_blocks(S, exp, hist):
    """12288-byte blocks: a chunk is 5461 whole blocks (67 104 768 bytes, not 64 MiB); the same
    block on both sides of the chunk edge."""
    bb = 12288
    per = HOST_CHUNK // bb
    assert (per, per * bb) == (5461, 67104768)
    size = (per + 2) * bb + 100
    a = exp.dgen(size, 2, 2).copy()
    same = np.random.default_rng(6000).integers(0, 256, bb, dtype=np.uint8)
    a[(per - 1) * bb:per * bb] = same
    a[per * bb:(per + 1) * bb] = same
    want = expect(S, [a], bb, hist=hist)
    assert (want.bytes, want.blocks) == (size, per + 3)         # the 100-byte tail is the last one
    assert S.measure_data(a, block_bytes=bb, hist=hist) == want
    if not hist:   # apart, the two blocks are one block more: the pair was counted once across the edge
        a[per * bb] ^= 1
        apart = expect(S, [a], bb)
        assert apart.unique_blocks == want.unique_blocks + 1
        assert S.measure_data(a, block_bytes=bb) == apart


OWN_BB = HOST_CHUNK + 4096
OWN_RUNS = ((0, 4096), (HOST_CHUNK - 16, HOST_CHUNK + 16), (OWN_BB - 16, OWN_BB))


def own_block(seed):
    """A block larger than the staging chunk: zeros, with non-zero random bytes at its start,
    around offset 64 MiB and at its end."""
    rng = np.random.default_rng(seed)
    b = np.zeros(OWN_BB, np.uint8)
    for lo, hi in OWN_RUNS:
        b[lo:hi] = rng.integers(1, 256, hi - lo, dtype=np.uint8)
    return b


@pytest.mark.parametrize("case", ["short", "exact", "copy", "changed"])
def test_measure_data_blocks_above_the_chunk(S, case):
    """block_bytes = 64 MiB + 4096: the call stages through two device buffers of its own."""
    b = own_block(6100)
    nonzero = sum(hi - lo for lo, hi in OWN_RUNS)
    if case == "short":
        a, shape = b[:OWN_BB - 100], (1, 1, OWN_BB - 100 - (nonzero - 16))
    elif case == "exact":
        a, shape = b, (1, 1, OWN_BB - nonzero)
    else:
        a = np.concatenate([b, b, b[:4196]])
        shape = (3, 2, a.size - 2 * nonzero - 4096)
        if case == "changed":
            k = OWN_BB + HOST_CHUNK + 5                          # inside block 1's run around 64 MiB
            a[k] = a[k] % 255 + 1                                # another non-zero value
            shape = (3, 3, shape[2])
    want = expect(S, [a], OWN_BB, hist=True)
    assert (want.blocks, want.unique_blocks, want.zero_bytes) == shape
    assert S.measure_data(a, block_bytes=OWN_BB, hist=True) == want
