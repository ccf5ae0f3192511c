"""GPU: payload verification (k_verify_stream and the surfaces over it).

Expected bytes always come from the C oracle (oracle/oracle_c.py), never from
the library's own fill.  In sections 1-9 a corrupted byte is `^= 0xFF`, so it
always differs; sections 10-12 corrupt single bits, every 16-byte piece on its
own, and seeded random mixes, with the expected result taken from numpy
(`diff_expect`).  Every assertion is exact: byte count, block count and first
offset.
"""
import functools
import os
import random
import threading

import numpy as np
import pytest

from oracle import oracle_py as P

pytestmark = pytest.mark.gpu
SOAK = max(1, int(os.environ.get("S3DG_FUZZ_SOAK", "1")))   # soak runs: seeds x SOAK

BLK = 4096
SIZES = [1, 15, 16, 17, 31, 32, 33, 2047, 2048, 2049, 4095, 4096, 4097, 8292, 3 * 4096 + 2080]
DEDUPS = [1, 2, 3]
# 128: c = 4064, the window is the block's last 32 bytes; 200: c = 4075/4076,
# a window of fewer than 32 bytes (the next_u32 tail path)
COMPRESS = [1, 2, 3, (3, 2), 128, 200]
HOST_CHUNK = 64 << 20          # the host path's staging chunk (s3dg_host.cpp kChunk)
OTHER_BASE_SEED = 0x0123456789ABCDEF


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
    """One context per waves-per-block setting (the shared context stays as it is)."""
    ctxs = {w: S.Context(0, base_seed=S.DEFAULT_BASE_SEED, waves_per_block=w) for w in (1, 2, 4)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module")
def exp(S, oracle, base):
    """Oracle bytes, computed once per argument set and never modified (callers copy)."""
    @functools.lru_cache(maxsize=None)
    def controlled(size, dedup, compress, entropy, base_seed=None):
        fn, fd = S.compress_ratio(compress)
        b = base if base_seed is None else oracle.base_block(base_seed)
        a = oracle.fill_controlled(size, dedup, fn, fd, entropy, b)
        a.setflags(write=False)
        return a

    @functools.lru_cache(maxsize=None)
    def random(size, entropy):
        a = oracle.random_data(size, entropy, base)
        a.setflags(write=False)
        return a

    class E:
        pass
    E.controlled, E.random = staticmethod(controlled), staticmethod(random)
    return E


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to("cuda:0")


def flipped(a, positions):
    b = np.array(a, dtype=np.uint8, copy=True)
    for p in positions:
        b[p] ^= 0xFF
    return b


def diff_expect(S, got, want):
    """The result of verifying `got` against `want`, from numpy, per 4 KiB block."""
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return S.VerifyResult()
    return S.VerifyResult(int(bad.size), int(np.unique(bad // BLK).size), int(bad[0]))


# ---- 1. single objects, clean ---------------------------------------------------

@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("compress", COMPRESS, ids=str)
def test_clean_controlled(S, torch, wave_ctx, exp, waves, compress):
    ctx = wave_ctx[waves]
    for size in SIZES:
        for dedup in DEDUPS:
            want = exp.controlled(size, dedup, compress, 42)
            t = dev(torch, want)
            r = ctx.verify_controlled(t, size, dedup, compress, entropy=42)
            assert r == S.VerifyResult() and r.ok and r.first_offset is None, (size, dedup, r)
            assert np.array_equal(t.cpu().numpy(), want), (size, dedup)     # read-only pass


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_clean_random(S, torch, wave_ctx, exp, waves):
    ctx = wave_ctx[waves]
    for size in SIZES:
        want = exp.random(size, 7)
        t = dev(torch, want)
        r = ctx.verify_random_data(t, size, entropy=7)
        assert r == S.VerifyResult(), (size, r)
        assert np.array_equal(t.cpu().numpy(), want), size
        if size > 1:                                  # and it is not vacuous
            bad = flipped(want, [size - 1])
            assert ctx.verify_random_data(dev(torch, bad), size, entropy=7) == S.VerifyResult(1, 1, size - 1)


# ---- 2. one flipped byte at each boundary the kernel distinguishes -----------------

def _boundary_positions(S, size, dedup, compress):
    """name -> byte offset, for block 1 (a full block) of the object and its edges."""
    fn, fd = S.compress_ratio(compress)
    nb = (size + BLK - 1) // BLK
    U = S.unique_blocks(nb, dedup)
    assert U < nb and nb >= 4 and size % BLK
    u = 1 % U
    tot = fn * BLK
    c = tot // fd + (((u + 1) * (tot % fd)) // fd - (u * (tot % fd)) // fd)   # src/data_gen.rs:177-190
    so = max(c, BLK // 2)
    b1 = BLK
    pos = {"block byte 0": b1, "last zero byte": b1 + c - 1, "first window byte": b1 + c,
           "c+31": b1 + c + 31, "c+32": b1 + c + 32, "so": b1 + so, "so+31": b1 + so + 31,
           "base image byte": b1 + 4000, "last byte of a full block": 2 * BLK - 1,
           "last byte of the ragged tail": size - 1, "dedup block": U * BLK + 100}
    assert c >= 1 and so + 32 < 4000 and U * BLK + 100 < size
    return pos


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("compress", [3, (3, 2)], ids=str)   # 3: so == c; 3/2: window 2 apart at 2048
def test_single_flips(S, torch, wave_ctx, exp, waves, compress):
    ctx = wave_ctx[waves]
    size, dedup = 3 * BLK + 2080, 2
    want = exp.controlled(size, dedup, compress, 42)
    pos = _boundary_positions(S, size, dedup, compress)
    for name, p in pos.items():
        r = ctx.verify_controlled(dev(torch, flipped(want, [p])), size, dedup, compress, entropy=42)
        assert r == S.VerifyResult(1, 1, p), (name, p, r)
    allp = sorted(set(pos.values()))
    r = ctx.verify_controlled(dev(torch, flipped(want, allp)), size, dedup, compress, entropy=42)
    assert r == S.VerifyResult(len(allp), len({p // BLK for p in allp}), allp[0]), r


# ---- 3. wrong parameters -------------------------------------------------------------

@pytest.mark.parametrize("waves", [1, 2, 4])
def test_wrong_parameters(S, torch, wave_ctx, exp, waves):
    ctx = wave_ctx[waves]
    size, ent, dedup, comp = 64 * BLK + 100, 42, 2, 3
    data = exp.controlled(size, dedup, comp, ent)
    t = dev(torch, data)
    assert ctx.verify_controlled(t, size, dedup, comp, entropy=ent).ok
    for (e2, d2, c2) in [(ent + 1, dedup, comp), (ent, dedup + 1, comp), (ent, dedup, 2), (ent, dedup, (3, 2))]:
        want = diff_expect(S, data, exp.controlled(size, d2, c2, e2))
        assert want.mismatched_blocks >= 32
        r = ctx.verify_controlled(t, size, d2, c2, entropy=e2)
        assert r == want, ((e2, d2, c2), r, want)
    # every block wrong (another base block): all workgroups hit the same three words
    other = S.Context(0, base_seed=OTHER_BASE_SEED, waves_per_block=waves)
    try:
        want = diff_expect(S, data, exp.controlled(size, dedup, comp, ent, OTHER_BASE_SEED))
        assert want.mismatched_blocks == 64   # all 64 full blocks; the 100-byte tail is zero prefix only
        assert other.verify_controlled(t, size, dedup, comp, entropy=ent) == want
    finally:
        other.close()
    assert np.array_equal(t.cpu().numpy(), data)


# ---- 4. range -------------------------------------------------------------------------

def test_range(S, torch, gpu_ctx, exp):
    size, dedup, comp, ent = 10 * BLK + 100, 2, 3, 9
    obj = exp.controlled(size, dedup, comp, ent)
    lo, hi = 3, 7
    inside = 5 * BLK + 2900
    outside = 8 * BLK + 17
    bad = flipped(obj, [outside])                       # a flip the range does not hold
    t = dev(torch, bad[lo * BLK:hi * BLK])
    assert gpu_ctx.verify_range(t, size, lo, hi, dedup, comp, ent) == S.VerifyResult()
    bad = flipped(bad, [inside])
    t = dev(torch, bad[lo * BLK:hi * BLK])
    assert gpu_ctx.verify_range(t, size, lo, hi, dedup, comp, ent) == S.VerifyResult(1, 1, inside - lo * BLK)
    # the range holding the ragged last block (blk_hi past the end is clipped)
    tail = obj[9 * BLK:]
    assert tail.size == BLK + 100
    assert gpu_ctx.verify_range(dev(torch, tail), size, 9, 99, dedup, comp, ent) == S.VerifyResult()
    r = gpu_ctx.verify_range(dev(torch, flipped(tail, [0, tail.size - 1])), size, 9, 11, dedup, comp, ent)
    assert r == S.VerifyResult(2, 2, 0)
    r = gpu_ctx.verify_range(dev(torch, flipped(tail, [tail.size - 1])), size, 9, 11, dedup, comp, ent)
    assert r == S.VerifyResult(1, 1, BLK + 99)
    assert gpu_ctx.verify_range(dev(torch, tail), size, 4, 4, dedup, comp, ent) == S.VerifyResult()   # empty range


# ---- 5. stream, basic -------------------------------------------------------------------

def test_stream_basic(S, torch, gpu_ctx, oracle, base):
    size, n, first, seed = 2 * BLK + 100, 3, 5, 0x5EED0000000000AB
    stride = ((size + 15) & ~15) + 32
    fn, fd = S.compress_ratio(2)
    want = oracle.fill_stream(size, n, 2, fn, fd, seed, first, base, stride)
    args = dict(obj_size=size, n_objs=n, stride=stride, dedup=2, compress=2, seed_base=seed, first_obj=first)
    assert gpu_ctx.verify_stream(dev(torch, want), **args) == S.VerifyResult()
    junk = want.copy()
    for j in range(n):                                   # the gaps are never read
        junk[j * stride + size:(j + 1) * stride] = 0xA5
    assert gpu_ctx.verify_stream(dev(torch, junk), **args) == S.VerifyResult()
    p = BLK + 2050
    r = gpu_ctx.verify_stream(dev(torch, flipped(junk, [2 * stride + p])), **args)
    assert r == S.VerifyResult(1, 1, 2 * stride + p)
    r = gpu_ctx.verify_stream(dev(torch, flipped(junk, [stride + size - 1, 2 * stride + 3])), **args)
    assert r == S.VerifyResult(2, 2, stride + size - 1)
    # the same objects under another first_obj are other payloads
    assert not gpu_ctx.verify_stream(dev(torch, want), **dict(args, first_obj=first + 1)).ok
    # a tensor too small for the call's reads is refused before the launch
    with pytest.raises(ValueError, match="reads"):
        gpu_ctx.verify_stream(dev(torch, want)[:-1 - (stride - size)], **args)
    with pytest.raises(ValueError, match="aligned"):
        gpu_ctx.verify_stream(dev(torch, want), **dict(args, stride=stride + 8))


# ---- 6. stream crossing the 65 535-object launch split -----------------------------------

def test_stream_launch_split(S, torch, gpu_ctx, oracle, base):
    size, n, seed = 48, 65539, 0xABCDEF
    fn, fd = S.compress_ratio(1)
    want = oracle.fill_stream(size, n, 1, fn, fd, seed, 0, base)
    args = dict(obj_size=size, n_objs=n, seed_base=seed)
    assert gpu_ctx.verify_stream(dev(torch, want), **args) == S.VerifyResult()
    p = 65537 * size + 5
    assert gpu_ctx.verify_stream(dev(torch, flipped(want, [p])), **args) == S.VerifyResult(1, 1, p)
    q = 65534 * size + 47                                 # last object of the first launch
    assert gpu_ctx.verify_stream(dev(torch, flipped(want, [p, q])), **args) == S.VerifyResult(2, 2, q)


def test_stream_offsets_past_4gib(S, torch, gpu_ctx, oracle, base):
    """Object 1 starts past 2^32 bytes: offsets are 64-bit end to end.  The gap
    between the two objects is never read, so it is left uninitialised."""
    size, seed = 2 * BLK + 100, 77
    stride = (1 << 32) + BLK
    fn, fd = S.compress_ratio(3)
    objs = oracle.fill_stream(size, 2, 1, fn, fd, seed, 0, base)
    t = torch.empty(stride + size, dtype=torch.uint8, device="cuda:0")
    t[:size] = dev(torch, objs[:size])
    t[stride:] = dev(torch, objs[size:])
    args = dict(obj_size=size, n_objs=2, stride=stride, compress=3, seed_base=seed)
    assert gpu_ctx.verify_stream(t, **args) == S.VerifyResult()
    p = BLK + 3000
    t[stride + p] ^= 0xFF
    assert gpu_ctx.verify_stream(t, **args) == S.VerifyResult(1, 1, stride + p)
    del t
    torch.cuda.empty_cache()


# ---- 7. two host threads, one context ------------------------------------------------------

def test_two_threads_two_streams(S, torch, gpu_ctx, exp):
    size, dedup, comp, ent = 64 * BLK + 100, 1, 2, 3
    want = exp.controlled(size, dedup, comp, ent)
    flips = [5, BLK + 2048, BLK + 2049, 40 * BLK, size - 1]
    bufs = [dev(torch, want), dev(torch, flipped(want, flips))]
    expect = [S.VerifyResult(), S.VerifyResult(5, 4, 5)]
    torch.cuda.synchronize()
    got, errs = [[], []], []

    def run(k):
        try:
            st = torch.cuda.Stream(device=0)
            for _ in range(20):
                got[k].append(gpu_ctx.verify_controlled(bufs[k], size, dedup, comp, entropy=ent, stream=st))
            gpu_ctx.release_stream(st)
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(2):
        assert got[k] == [expect[k]] * 20, k


# ---- 8. host buffers -------------------------------------------------------------------------

def _unaligned(a):
    """The bytes of `a` in a buffer that starts one byte past an allocation."""
    buf = bytearray(1 + a.size)
    mv = memoryview(buf)[1:]
    mv[:] = a.tobytes()
    return mv


@pytest.mark.parametrize("base_seed", [None, OTHER_BASE_SEED], ids=["default-base", "caller-base"])
@pytest.mark.parametrize("size,flips", [(1, [0]), (4097, [4095, 4096]),
                                        (HOST_CHUNK + BLK + 123, [HOST_CHUNK - 1, HOST_CHUNK, HOST_CHUNK + BLK + 122])])
def test_host_buffers(S, oracle, exp, size, flips, base_seed):
    dedup, comp, ent = 2, 3, 11
    want = exp.controlled(size, dedup, comp, ent, base_seed)
    bb = None if base_seed is None else oracle.base_block(base_seed).tobytes()
    kw = dict(dedup=dedup, compress=comp, entropy=ent, base_block=bb)
    assert S.verify_controlled_data_seeded(want.tobytes(), **kw) == S.VerifyResult()      # read-only bytes
    mv = _unaligned(want)
    assert S.verify_controlled_data_seeded(mv, **kw) == S.VerifyResult()
    for p in flips:
        mv[p] ^= 0xFF
        assert S.verify_controlled_data_seeded(mv, **kw) == S.VerifyResult(1, 1, p), p
        mv[p] ^= 0xFF
    for p in flips:
        mv[p] ^= 0xFF
    r = S.verify_controlled_data_seeded(mv, **kw)
    assert r == S.VerifyResult(len(flips), len({p // BLK for p in flips}), flips[0])
    if base_seed is not None and size > 1:   # the caller's block matters
        assert not S.verify_controlled_data_seeded(want.tobytes(), dedup, comp, ent).ok


def test_host_read_only_mapping(S, exp, tmp_path):
    """Pages the process cannot write (a PROT_READ file mapping), unaligned length."""
    import mmap
    size = 3 * BLK + 5
    want = exp.controlled(size, 2, 3, 11)
    path = tmp_path / "ro.bin"
    path.write_bytes(flipped(want, [size - 1]).tobytes())
    with open(path, "rb") as f:
        m = mmap.mmap(f.fileno(), size, prot=mmap.PROT_READ)
        try:
            assert S.verify_controlled_data_seeded(m, 2, 3, 11) == S.VerifyResult(1, 1, size - 1)
        finally:
            m.close()


# ---- 9. files ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,comp", [("controlled", 2), ("random", 1)])
def test_files(S, gpu_ctx, oracle, base, tmp_path, kind, comp):
    n, size, seed = 5, 3 * BLK + 7, 0xF11E
    uris = [f"file://{tmp_path}/objs/o-{j}" for j in range(n)]
    cfg = S.Config.new_with_defaults("RAW", 1, size, 1, comp)
    S.put_objects(uris, size, 4, cfg, seed=seed, payload=kind, context=gpu_ctx)
    path = lambda j: f"{tmp_path}/objs/o-{j}"   # noqa: E731
    fn, fd = S.compress_ratio(comp)
    e2 = oracle.object_entropy(seed, 2)
    want2 = oracle.fill_controlled(size, 1, fn, fd, e2, base) if kind == "controlled" else oracle.random_data(size, e2, base)
    assert open(path(2), "rb").read() == want2.tobytes()
    kw = dict(config=cfg, seed=seed, payload=kind, context=gpu_ctx)
    res = S.verify_objects(uris, size, **kw)
    assert res.ok and res.mismatches == [] and (res.objects, res.bytes) == (n, n * size)
    assert not S.verify_objects(uris, size, **dict(kw, seed=seed + 1)).ok
    p = 2 * BLK + 33
    with open(path(3), "r+b") as f:
        f.seek(p)
        b = f.read(1)
        f.seek(p)
        f.write(bytes([b[0] ^ 0xFF]))
    res = S.verify_objects(uris, size, **kw)
    assert res.mismatches == [(3, S.VerifyResult(1, 1, p))]
    assert (res.mismatched_objects, res.mismatched_bytes, res.mismatched_blocks) == (1, 1, 1)
    os.truncate(path(1), size - 10)
    res = S.verify_objects(uris, size, **kw)
    assert [j for j, _ in res.mismatches] == [1, 3]
    r1 = res.mismatches[0][1]
    # 10 missing bytes, in blocks 2 and 3 (the object's last 7 bytes are block 3)
    assert r1 == S.VerifyResult(10, 2, size - 10)
    assert res.mismatches[1] == (3, S.VerifyResult(1, 1, p))
    with open(path(0), "ab") as f:                         # a file that is too long
        f.write(b"xyz")
    res = S.verify_objects(uris[:1], size, **kw)
    assert res.mismatches == [(0, S.VerifyResult(3, 1, size))]


# ---- 10. every bit of a byte -----------------------------------------------------------------------

@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("compress", [3, (3, 2)], ids=str)
def test_every_bit(S, torch, wave_ctx, exp, waves, compress):
    """diff_piece folds a byte's eight bits into one: a byte that differs in
    bit b only, for each b, is counted once.  Two bytes of one piece, the four
    bytes of one dword and all sixteen bytes of one piece, in the zero prefix,
    across the window's start and in the base image of block 1."""
    ctx = wave_ctx[waves]
    size, dedup = 3 * BLK + 2080, 2
    want = exp.controlled(size, dedup, compress, 42)
    fn, fd = S.compress_ratio(compress)
    c = P.const_len(1 % S.unique_blocks(4, dedup), fn, fd)
    assert 32 < c < 3000
    for piece in (10, c // 16, 250):
        o = BLK + 16 * piece
        patterns = {2: [o + 3, o + 12], 4: [o + 8, o + 9, o + 10, o + 11], 16: list(range(o, o + 16))}
        for bit in range(8):
            for count, pos in patterns.items():
                bad = np.array(want, dtype=np.uint8, copy=True)
                bad[pos] ^= 1 << bit
                want_r = diff_expect(S, bad, want)
                assert want_r == S.VerifyResult(count, 1, pos[0])
                r = ctx.verify_controlled(dev(torch, bad), size, dedup, compress, entropy=42)
                assert r == want_r, (piece, bit, count, r)


# ---- 11. every 16-byte piece, on its own --------------------------------------------------------------

@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("compress", [3, (3, 2)], ids=str)
def test_every_piece(S, torch, wave_ctx, exp, waves, compress):
    """One full block, then a ragged block whose last piece holds 5 bytes: each
    piece is shown one flipped bit (bit p % 8 of byte p % 16 of piece p), so
    every lane that owns a piece at this waves-per-block setting reports."""
    ctx = wave_ctx[waves]
    size, dedup = BLK + 2085, 1
    want = exp.controlled(size, dedup, compress, 42)
    npieces = (size + 15) // 16
    assert size % 16 == 5 and npieces == 256 + 131
    flips = [(min(16 * p + p % 16, size - 1), 1 << (p % 8)) for p in range(npieces)]
    assert len({pos for pos, _ in flips}) == npieces
    t = dev(torch, want)
    assert ctx.verify_controlled(t, size, dedup, compress, entropy=42) == S.VerifyResult()
    for p, (pos, mask) in enumerate(flips):
        t[pos] ^= mask
        r = ctx.verify_controlled(t, size, dedup, compress, entropy=42)
        t[pos] ^= mask
        assert r == S.VerifyResult(1, 1, pos), (p, pos, r)
    assert np.array_equal(t.cpu().numpy(), want)
    bad = np.array(want, dtype=np.uint8, copy=True)
    for pos, mask in flips:
        bad[pos] ^= mask
    want_r = diff_expect(S, bad, want)
    assert want_r == S.VerifyResult(npieces, 2, flips[0][0])
    assert ctx.verify_controlled(dev(torch, bad), size, dedup, compress, entropy=42) == want_r


# ---- 12. seeded fuzz ------------------------------------------------------------------------------------

def _fuzz_size(rnd):                      # as tests/test_gpu_fuzz.py::_size
    k = rnd.random()
    if k < 0.3:
        return rnd.randint(1, 5000)
    if k < 0.6:
        return rnd.choice([4096, 8192, 2048, 2049, 2047]) * rnd.randint(1, 40) + rnd.randint(-7, 7)
    return rnd.randint(5000, 6 << 20)


FUZZ_COMPRESS = [1, 1, 2, 3, 4, 7, 16, (3, 2), (5, 3), (9, 4),
                 P.wide_compress(43690, 65537), P.wide_compress(1431694211, 4294967291)]


def _corrupt(rnd, a):
    """Corrupt the object `a` (a writable copy of the oracle's bytes) in place
    by a random mix; what differs afterwards is numpy's to say."""
    n = a.size
    mode = rnd.choice(["none", "bits", "bytes", "runs", "mix", "mix"])
    if mode in ("bits", "mix"):
        for _ in range(rnd.randint(1, 8)):
            a[rnd.randrange(n)] ^= 1 << rnd.randrange(8)
    if mode in ("bytes", "mix"):
        for _ in range(rnd.randint(1, 8)):
            a[rnd.randrange(n)] = rnd.randrange(256)      # may be the value already there
    if mode in ("runs", "mix"):
        for _ in range(rnd.randint(1, 3)):
            ln = rnd.randint(1, 40)
            edge = rnd.choice([16 * rnd.randint(0, n // 16), BLK * rnd.randint(0, n // BLK), n])
            lo = max(0, min(edge - rnd.randint(0, ln), n - 1))      # the run straddles or touches `edge`
            hi = min(n, lo + ln)                                    # and stops at the object's end
            a[lo:hi] = np.frombuffer(rnd.randbytes(hi - lo), np.uint8)
    return mode


@pytest.mark.parametrize("seed", range(8 * SOAK))
def test_fuzz_verify(S, torch, gpu_ctx, oracle, seed):
    rnd = random.Random(4000 + seed)
    orig = gpu_ctx.base_block
    base = np.frombuffer(rnd.randbytes(BLK), np.uint8).copy()
    gpu_ctx.set_base_block(base.tobytes())
    try:
        for _ in range(4):
            gpu_ctx.set_waves_per_block(rnd.choice([0, 1, 2, 4]))
            d, c = rnd.choice([0, 1, 2, 3, 5, 64]), rnd.choice(FUZZ_COMPRESS)
            fn, fd = S.compress_ratio(c)
            assert (fn, fd) == P.compress_ratio(c)
            # one object
            L, e = _fuzz_size(rnd), rnd.getrandbits(64)
            want = oracle.fill_controlled(L, d, fn, fd, e, base)
            got = want.copy()
            mode = _corrupt(rnd, got)
            r = gpu_ctx.verify_controlled(dev(torch, got), L, d, c, entropy=e)
            assert r == diff_expect(S, got, want), ("controlled", L, d, c, e, mode, r)
            # the random-data layout
            L, e = _fuzz_size(rnd), rnd.getrandbits(64)
            want = oracle.random_data(L, e, base)
            got = want.copy()
            mode = _corrupt(rnd, got)
            r = gpu_ctx.verify_random_data(dev(torch, got), L, entropy=e)
            assert r == diff_expect(S, got, want), ("random", L, e, mode, r)
            # a block range of an object
            L, e = _fuzz_size(rnd), rnd.getrandbits(64)
            nb = (L + BLK - 1) // BLK
            lo = rnd.randrange(nb)
            hi = rnd.randint(lo + 1, nb + 2)
            want = oracle.fill_controlled_range(L, lo, hi, d, fn, fd, e, base)
            got = want.copy()
            mode = _corrupt(rnd, got)
            r = gpu_ctx.verify_range(dev(torch, got), L, lo, hi, d, c, e)
            assert r == diff_expect(S, got, want), ("range", L, lo, hi, d, c, e, mode, r)
            # a stream at a padded stride, the gaps poisoned
            n, sz = rnd.randint(1, 9), _fuzz_size(rnd) % (1 << 20) + 1
            stride = (sz + 15) // 16 * 16 + 16 * rnd.randint(0, 3)
            sb, first = rnd.getrandbits(64), rnd.randint(0, 1 << 20)
            buf = np.frombuffer(rnd.randbytes(n * stride), np.uint8).copy()
            nbytes, nblocks, first_bad, modes = 0, 0, None, []
            for j in range(n):
                want = oracle.fill_controlled(sz, d, fn, fd, P.object_entropy(sb, first + j), base)
                got = want.copy()
                modes.append(_corrupt(rnd, got))
                buf[j * stride:j * stride + sz] = got
                one = diff_expect(S, got, want)
                nbytes += one.mismatched_bytes
                nblocks += one.mismatched_blocks
                if first_bad is None and not one.ok:
                    first_bad = j * stride + one.first_offset
            want_r = S.VerifyResult(nbytes, nblocks, first_bad)
            r = gpu_ctx.verify_stream(dev(torch, buf), obj_size=sz, n_objs=n, stride=stride, dedup=d, compress=c,
                                      seed_base=sb, first_obj=first)
            assert r == want_r, ("stream", sz, n, stride, d, c, sb, first, modes, r, want_r)
    finally:
        gpu_ctx.set_base_block(orig)
        gpu_ctx.set_waves_per_block(0)
