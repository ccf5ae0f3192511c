"""GPU: zero-prefix ratios with denominators around and above 2^16 through
every consumer of the prefix parameters.

plan_block's closed form of src/data_gen.rs:174-190 has a 32-bit product arm
(f_den <= 65536) and a 64-bit arm above it; the wide ratios (oracle_py.
WIDE_RATIOS) sit on both sides of that boundary and run up to the largest
32-bit denominator, where `r0 + rem` passes 2^32.  Every comparison is byte
for byte against the C oracle (oracle/s3dg_oracle.c, the reference's literal
accumulator), with guard bytes around every output.
"""
import numpy as np
import pytest

from oracle import oracle_py as P

pytestmark = pytest.mark.gpu

BLK = 4096
MiB = 1 << 20
GUARD = 0xA7
# every compress argument of the table: the 21 ratios as (p, q) tuples, then
# the reference-semantics integers
WIDE = [P.wide_compress(fn, fd) for fn, fd in P.WIDE_RATIOS] + P.WIDE_INTS


def _row(f_den):
    return [P.wide_compress(fn, fd) for fn, fd in P.WIDE_RATIOS if fd == f_den]


def _cid(c):
    return f"{c[0] - c[1]}/{c[0]}" if isinstance(c, tuple) else f"c{c}"


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


def _ratio(S, c):
    """(f_num, f_den) as the library maps `c`, checked against the oracle's rule."""
    r = S.compress_ratio(c)
    assert r == P.compress_ratio(c), c
    return r


def _guarded(torch, n, tail=48):
    return torch.full((n + tail,), GUARD, dtype=torch.uint8, device="cuda")


def _dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to("cuda:0")


def _diff_expect(S, got, want):
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return S.VerifyResult()
    return S.VerifyResult(int(bad.size), int(np.unique(bad // BLK).size), int(bad[0]))


def _first_window_byte(blk_lo, nblk, length, U, fn, fd):
    """Offset (from block blk_lo) of the first window byte of the first block
    of the range that has a window; the range's last byte when every block is
    zero prefix only."""
    for k in range(nblk):
        i = blk_lo + k
        L = min(BLK, length - i * BLK)
        c = P.const_len(i % U, fn, fd)
        if c < L:
            return k * BLK + c
    return min((blk_lo + nblk) * BLK, length) - blk_lo * BLK - 1


def _one_bit(want, pos, bit):
    b = np.array(want, dtype=np.uint8, copy=True)
    b[pos] ^= 1 << bit
    return b


# ---- fill_controlled / verify_controlled ---------------------------------------------

LENGTHS = [1, 2049, 4096, 4097, 16 * BLK + 2080, 64 * BLK + 5]


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("compress", WIDE, ids=_cid)
def test_fill_and_verify_controlled(S, torch, oracle, base, wave_ctx, waves, compress):
    ctx = wave_ctx[waves]
    fn, fd = _ratio(S, compress)
    for n in LENGTHS:
        for dedup in (1, 3):
            e = 0xC0FFEE0000 + n
            want = oracle.fill_controlled(n, dedup, fn, fd, e, base)
            t = _guarded(torch, n)
            ctx.fill_controlled(t, n, dedup=dedup, compress=compress, entropy=e)
            h = t.cpu().numpy()
            assert np.array_equal(h[:n], want), (n, dedup)
            assert (h[n:] == GUARD).all(), (n, dedup)
            # verify: the oracle's bytes are clean, one flipped bit is found exactly
            assert ctx.verify_controlled(_dev(torch, want), n, dedup, compress, entropy=e) == S.VerifyResult(), (n, dedup)
            nb = -(-n // BLK)
            pos = _first_window_byte(0, nb, n, P.unique_blocks(nb, dedup), fn, fd)
            bad = _one_bit(want, pos, (n + dedup) % 8)
            r = ctx.verify_controlled(_dev(torch, bad), n, dedup, compress, entropy=e)
            assert r == _diff_expect(S, bad, want) == S.VerifyResult(1, 1, pos), (n, dedup, pos, r)


# ---- fill_stream: the 2D kernel and the tiled kernel ------------------------------------

@pytest.mark.parametrize("compress", _row(65536) + _row(65537) + _row(4294967291), ids=_cid)
def test_fill_stream_2d(S, torch, oracle, base, gpu_ctx, compress):
    fn, fd = _ratio(S, compress)
    size, n, seed, first = 17 * BLK + 100, 9, 0x5EED0000000000CD, 3
    stride = ((size + 15) & ~15) + 48
    for dedup in (1, 3):
        t = _guarded(torch, n * stride)
        gpu_ctx.fill_stream(t, obj_size=size, n_objs=n, stride=stride, dedup=dedup, compress=compress,
                            seed_base=seed, first_obj=first)
        h = t.cpu().numpy()
        exp = oracle.fill_stream(size, n, dedup, fn, fd, seed, first, base, stride=stride)
        for j in range(n):
            o = j * stride
            assert np.array_equal(h[o:o + size], exp[o:o + size]), (j, dedup)
            assert (h[o + size:o + stride] == GUARD).all(), (j, dedup)
        assert (h[n * stride:] == GUARD).all()


@pytest.mark.parametrize("compress,dedup", [(_row(65536)[1], 1), (_row(65537)[2], 3), (_row(4294967291)[0], 1)],
                         ids=["65536-d1", "65537-d3", "4294967291-d1"])
def test_fill_stream_tiled(S, torch, oracle, base, gpu_ctx, compress, dedup):
    """64 objects of 1 MiB + 123 (16 448 blocks) take the tiled batch kernel."""
    fn, fd = _ratio(S, compress)
    size, n, seed, first = MiB + 123, 64, 0x5EED0000000000EF, 1 << 20
    stride = MiB + 32768
    assert stride % 32768 == 0 and n * (-(-size // BLK)) >= 16384
    try:
        gpu_ctx.set_stream_tiles(1)
        t = _guarded(torch, n * stride)
        gpu_ctx.fill_stream(t, obj_size=size, n_objs=n, stride=stride, dedup=dedup, compress=compress,
                            seed_base=seed, first_obj=first)
        h = t.cpu().numpy()
    finally:
        gpu_ctx.set_stream_tiles(-1)
    exp = oracle.fill_stream(size, n, dedup, fn, fd, seed, first, base, stride=stride, threads=8)
    g = h[:n * stride].reshape(n, stride)
    assert np.array_equal(g[:, :size], exp.reshape(n, stride)[:, :size])
    assert (g[:, size:] == GUARD).all() and (h[n * stride:] == GUARD).all()


# ---- fill_batch: the prefix parameters are made on the device ---------------------------

BATCH_SIZES = [1, 17, 2049, 4096, 4097, 8191, 12288 + 2730, 16 * BLK + 2080, 17 * BLK, 20 * BLK + 1,
               24 * BLK + 4095, 31 * BLK + 7, 32 * BLK, 33 * BLK + 2048, 40 * BLK + 33, 47 * BLK + 5, 50 * BLK,
               56 * BLK + 2081, 61 * BLK + 9, 64 * BLK + 5, 65 * BLK, 70 * BLK + 4064, 72 * BLK + 100, 74 * BLK + 1,
               300 * 1024]


@pytest.mark.parametrize("tile", [0, 2, 64])
def test_fill_batch_device_prefix(S, torch, oracle, base, gpu_ctx, tile):
    assert len(BATCH_SIZES) == len(WIDE)
    rot = {0: 0, 2: 9, 64: 17}[tile]          # each tile setting pairs the ratios with other sizes
    objs, off = [], 0
    for k, size in enumerate(BATCH_SIZES):
        c = WIDE[(k + rot) % len(WIDE)]
        objs.append((off, size, 0xBA7C000000000000 + (k << 33) + tile, [0, 1, 2, 5][(k + tile) % 4], c))
        off += ((size + 15) & ~15) + 16 * (1 + k % 3)
    t = _guarded(torch, off, 16)
    try:
        gpu_ctx.set_batch_tile(tile)
        gpu_ctx.fill_batch(t, objs)
        h = t.cpu().numpy()
    finally:
        gpu_ctx.set_batch_tile(0)
    ends = [o[0] for o in objs[1:]] + [off + 16]
    for (o, size, e, d, c), end in zip(objs, ends):
        fn, fd = _ratio(S, c)
        assert np.array_equal(h[o:o + size], oracle.fill_controlled(size, d, fn, fd, e, base)), (size, d, c)
        assert (h[o + size:end] == GUARD).all(), (size, d, c)


# ---- fill_range / verify_range far into large objects --------------------------------------

NB_A = (1 << 17) + 3
NB_B = (1 << 24) + 3
# 131071 on object A as well: there up * rem passes 2^32 (up to 2^34), which it cannot below 65 538
RANGE_CASES = [(NB_A, fd, c) for fd in (65535, 65536, 65537, 131071) for c in _row(fd)] + \
              [(NB_B, fd, c) for fd in (1000003, 4294967291) for c in _row(fd)]


@pytest.mark.parametrize("dedup", [1, 3])
@pytest.mark.parametrize("nb,f_den,compress", RANGE_CASES, ids=lambda v: _cid(v) if isinstance(v, tuple) else str(v))
def test_range_at_large_block_indices(S, torch, oracle, base, gpu_ctx, nb, f_den, compress, dedup):
    """Object A (2^17 + 3 blocks): around block 65 536 the unique index passes
    f_den (u mod f_den wraps, and up * rem is at its largest on the 32-bit
    arm); object B (2^24 + 3 blocks): u * rem far past 2^32.  With dedup 3 the
    i mod U wrap lies inside a range."""
    fn, fd = _ratio(S, compress)
    assert fd == f_den
    length = (nb - 1) * BLK + 1234
    U = P.unique_blocks(nb, dedup)
    ranges = [(65530, 65546), (131060, 131075)] if nb == NB_A else [((1 << 24) - 8, (1 << 24) + 3)]
    if dedup == 3:
        ranges.append((U - 4, U + 4))
        assert any(lo < k * U < hi for lo, hi in ranges for k in (1, 2, 3))
    e = 2**64 - 7
    for lo, hi in ranges:
        want = oracle.fill_controlled_range(length, lo, hi, dedup, fn, fd, e, base)
        n = min(hi * BLK, length) - lo * BLK
        assert want.size == n <= 65536
        t = _guarded(torch, 65536)
        gpu_ctx.fill_range(t, length, lo, hi, dedup=dedup, compress=compress, entropy=e)
        h = t.cpu().numpy()
        assert np.array_equal(h[:n], want), (lo, hi)
        assert (h[n:] == GUARD).all(), (lo, hi)
        assert gpu_ctx.verify_range(_dev(torch, want), length, lo, hi, dedup, compress, e) == S.VerifyResult(), (lo, hi)
        pos = _first_window_byte(lo, hi - lo, length, U, fn, fd)
        bad = _one_bit(want, pos, lo % 8)
        r = gpu_ctx.verify_range(_dev(torch, bad), length, lo, hi, dedup, compress, e)
        assert r == S.VerifyResult(1, 1, pos), (lo, hi, pos, r)


# ---- DG1: zero prefix of floor(L * f_num / f_den) per 1 MiB block ----------------------------

@pytest.mark.parametrize("f_den", [65537, 1000003, 4294967291])
def test_dgen_fill(S, torch, oracle, f_den):
    """3 MiB + 5 in one keystream launch; 70 MiB split from one block up, so
    the zero-prefix launch runs too."""
    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    try:
        for k, compress in enumerate(_row(f_den)):
            fn, fd = _ratio(S, compress)
            for size, split in ((3 * MiB + 5, -1), (70 * MiB, 1)):
                ctx.set_dgen_zero_split(chunks=split)
                dedup, seed = 1 + k % 2, 0xD6E5000 + k
                t = _guarded(torch, size)
                ctx.dgen_fill(t, size, dedup=dedup, compress=compress, seed=seed)
                h = t.cpu().numpy()
                assert np.array_equal(h[:size], oracle.dgen_fill(size, dedup, fn, fd, seed)), (size, compress)
                assert (h[size:] == GUARD).all()
    finally:
        ctx.close()


# ---- host drop-in (integer compress, the reference's own argument) ------------------------------

def test_host_drop_in(S, oracle, base):
    size, dedup, comp, e = 3 * BLK + 5, 1, 100000, 0xABCDEF12345
    want = oracle.fill_controlled(size, dedup, comp - 1, comp, e, base)
    buf = bytearray([GUARD]) * (size + 64)
    S.fill_controlled_data_seeded(memoryview(buf)[:size], dedup, comp, e)
    assert np.array_equal(np.frombuffer(buf, np.uint8)[:size], want)
    assert bytes(buf[size:]) == bytes([GUARD]) * 64
    assert S.verify_controlled_data_seeded(want.tobytes(), dedup, comp, e) == S.VerifyResult()
    pos = _first_window_byte(0, 4, size, 4, comp - 1, comp)
    assert pos < size - 1
    bad = _one_bit(want, pos, 6)
    assert S.verify_controlled_data_seeded(bad.tobytes(), dedup, comp, e) == S.VerifyResult(1, 1, pos)
