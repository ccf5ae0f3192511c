"""GPU: the LZ4 size measurement (k_lz and the surfaces over it).

The judge is always the numpy restatement of the definition
(tests/lz_restatement.py) on host bytes: generated payloads are filled on the
GPU and copied back for it, crafted ones are built on the host.  All eight
fields are compared and every assertion is exact.
"""
import functools
import threading

import numpy as np
import pytest

import lz_cases as K
import lz_restatement as R

pytestmark = pytest.mark.gpu

BLK = 4096
MiB = 1 << 20
BLOCK_BYTES = [4096, 8192, 12288, 65536]
HOST_CHUNK = 64 << 20          # the host path's staging chunk


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to("cuda:0")


def host(t, n=None):
    a = t.cpu().numpy()
    return a if n is None else a[:n]


def want_of(objs, bb):
    return R.measure(objs, bb)


def check(ctx, torch, a, bb, note=None):
    """One object from host bytes: every field against the restatement."""
    a = np.ascontiguousarray(a, np.uint8)
    got = R.as_dict(ctx.measure_lz(dev(torch, a), block_bytes=bb))
    want = want_of([a], bb)
    assert got == want, (note, bb)
    assert got["literal_bytes"] + got["match_bytes"] == got["bytes"] == a.size
    return want


def same_hash_pair(rng):
    """Two different u32 with equal H, and a third value with another hash."""
    x = int(rng.integers(1 << 8, 1 << 32))
    hx = ((x * R.HASH_MUL) & 0xFFFFFFFF) >> 20
    ys = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
    hit = ys[(((ys * R.HASH_MUL) & 0xFFFFFFFF) >> 20 == hx) & (ys != x)]
    assert hit.size
    return x, int(hit[0])


def put32(a, pos, v):
    a[pos:pos + 4] = np.frombuffer(int(v).to_bytes(4, "little"), np.uint8)


# ---- 1. generated payloads ------------------------------------------------------------

GEN_SIZE = 2 * 65536 + 4096 + 37


@pytest.mark.parametrize("compress", [1, 2, 3, (3, 2), 128], ids=str)
@pytest.mark.parametrize("dedup", [1, 2, 4])
def test_controlled(S, torch, gpu_ctx, dedup, compress):
    t = torch.zeros(GEN_SIZE + 11, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.fill_controlled(t, GEN_SIZE, dedup=dedup, compress=compress, entropy=7)
    torch.cuda.synchronize()
    a = host(t, GEN_SIZE)
    for bb in BLOCK_BYTES:
        got = R.as_dict(gpu_ctx.measure_lz(t, GEN_SIZE, block_bytes=bb))
        assert got == want_of([a], bb), bb
    if compress == 1:
        # the repeated base block: nothing to a 4 KiB store, most of it to a 64 KiB one
        assert gpu_ctx.measure_lz(t, GEN_SIZE, block_bytes=4096).ratio == 1.0
        assert gpu_ctx.measure_lz(t, GEN_SIZE, block_bytes=65536).ratio > 8.0


@pytest.mark.parametrize("compress", [1, 2])
@pytest.mark.parametrize("dedup", [1, 3])
def test_dg1(S, torch, gpu_ctx, dedup, compress):
    n = MiB + 65536 + 100
    t = torch.zeros(n + 12, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.dgen_fill(t, n, dedup=dedup, compress=compress, seed=5)
    torch.cuda.synchronize()
    a = host(t, n)
    for bb in BLOCK_BYTES:
        got = gpu_ctx.measure_lz(t, n, block_bytes=bb)
        assert R.as_dict(got) == want_of([a], bb), bb
        if compress == 1:
            assert got.raw_blocks == got.blocks and got.ratio == 1.0
        else:
            assert got.ratio > 1.1


def test_keystream(S, torch, gpu_ctx):
    n = 2 * 65536 + 4096 + 100
    t = torch.zeros(n + 12, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.xoshiro_fill(t, n, chunk_bytes=65536, seed_base=3)
    torch.cuda.synchronize()
    a = host(t, n)
    for bb in BLOCK_BYTES:
        got = gpu_ctx.measure_lz(t, n, block_bytes=bb)
        assert R.as_dict(got) == want_of([a], bb), bb
        assert got.raw_blocks == got.blocks


# ---- 2. block-length edges ---------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 4, 5, 12, 13, 16, 17, 63, 64, 65])
def test_short_blocks(S, torch, gpu_ctx, n):
    rng = np.random.default_rng(100 + n)
    fills = [rng.integers(0, 256, n, dtype=np.uint8), np.full(n, 0x5A, np.uint8)]
    if n >= 13:
        fills.insert(0, np.zeros(n, np.uint8))      # a match is just possible
    for a in fills:
        pad = np.concatenate([a, np.full(-n % 16 + 16, 0xEE, np.uint8)])
        got = R.as_dict(gpu_ctx.measure_lz(dev(torch, pad), n, block_bytes=4096))
        assert got == want_of([a], 4096), n
    if n >= 13:
        assert want_of([np.zeros(n, np.uint8)], 4096)["matches"] == 1


@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_block_bytes_edges(S, torch, gpu_ctx, bb):
    rng = np.random.default_rng(200 + bb)
    for n in (bb - 1, bb, bb + 1, 2 * bb + 1):
        for a in (np.zeros(n, np.uint8), rng.integers(0, 4, n, dtype=np.uint8)):
            want = check(gpu_ctx, torch, a, bb, n)
            assert want["blocks"] == -(-n // bb)
    # n = bb + 1: the second block is one byte, stored raw
    w = want_of([np.zeros(bb + 1, np.uint8)], bb)
    assert (w["blocks"], w["raw_blocks"]) == (2, 1)


# ---- 3. crafted bytes ----------------------------------------------------------------------

def test_runs_of_five_at_every_offset(S, torch, gpu_ctx):
    """Five equal bytes at offsets 0-130 (both sides of two group edges), one object each."""
    rng = np.random.default_rng(300)
    n, stride = 300, 304
    objs = []
    for off in range(131):
        a = rng.integers(0, 256, n, dtype=np.uint8)
        a[off:off + 5] = 0x55
        a[off + 5] = 0x56
        if off:
            a[off - 1] = 0x57
        objs.append(a)
    buf = np.full(stride * len(objs), 0xEE, np.uint8)
    for j, a in enumerate(objs):
        buf[j * stride:j * stride + n] = a
    want = want_of(objs, 4096)
    assert want["matches"] >= 131
    got = gpu_ctx.measure_lz_stream(dev(torch, buf), n, len(objs), stride, block_bytes=4096)
    assert R.as_dict(got) == want
    for off in (0, 1, 62, 63, 64, 65, 127, 128, 130):     # and alone, so a wrong one has a name
        check(gpu_ctx, torch, objs[off], 4096, off)


@pytest.mark.parametrize("dist", [1, 63, 64, 65, 4096, 65528])
def test_repeat_at_distance(S, torch, gpu_ctx, dist):
    """The table sees earlier groups only; the restatement says which repeats are found."""
    rng = np.random.default_rng(400 + dist)
    n = min(dist + 8 + 30, 65536)
    ran = 0
    for start in (0, 3):
        if start + dist + 8 > n:
            continue
        a = rng.integers(0, 256, n, dtype=np.uint8)
        s = rng.integers(0, 256, 8, dtype=np.uint8)
        a[start:start + 8] = s
        a[start + dist:start + dist + 8] = s
        want = check(gpu_ctx, torch, a, 65536, (dist, start))
        ran += 1
        # Which distances hold a match at all.  63, 64, 65 and 4096 do, with the distance as the
        # offset (from the repeat's first byte, or a few bytes late where the source shares the
        # repeat's group or a colliding position displaced its entry).  1 and 65 528 do not, and
        # both parse as one literal run: at distance 1 the second write overlaps the first, so the
        # block holds nine random bytes and no repeat; at 65 528 the repeat starts at n - 8,
        # behind the last permitted match start n - 12 (and start = 3 does not fit the block).
        offsets = [off for _, off, _ in K.triples(R.parse_block(a))]
        assert (dist in offsets) == (dist in (63, 64, 65, 4096)), (dist, start)
        assert (want["matches"] >= 1) == (dist in (63, 64, 65, 4096)), (dist, start)
    assert ran == (1 if dist == 65528 else 2)
    found = {d: want_of([_repeat_block(d)], 65536)["matches"] for d in (63, 64, 65)}
    assert found[65] >= 1        # a whole group apart: always seen


def _repeat_block(dist):
    rng = np.random.default_rng(77)
    a = rng.integers(0, 256, dist + 40, dtype=np.uint8)
    a[dist:dist + 8] = a[0:8]
    return a


def test_displaced_candidate(S, torch, gpu_ctx):
    """x, then a colliding y in a later group, then x again: the table holds y, so the repeat is
    found one byte late, at the position whose word was not displaced; without y at its start."""
    rng = np.random.default_rng(500)
    x, y = same_hash_pair(rng)
    a = rng.integers(0, 256, 400, dtype=np.uint8)
    put32(a, 10, x)
    a[300:320] = a[10:30]
    plain = check(gpu_ctx, torch, a, 4096, "plain")
    b = a.copy()
    put32(b, 100, y)
    displaced = check(gpu_ctx, torch, b, 4096, "displaced")
    assert plain["matches"] == displaced["matches"] == 1
    assert plain["match_bytes"] == displaced["match_bytes"] + 1


def test_two_of_one_group_share_a_hash(S, torch, gpu_ctx):
    """x at 10 and the colliding y at 20, one group: position 20 is the next groups' candidate."""
    rng = np.random.default_rng(501)
    x, y = same_hash_pair(rng)
    base = rng.integers(0, 256, 400, dtype=np.uint8)
    put32(base, 10, x)
    put32(base, 20, y)
    a = base.copy()
    a[200:216] = a[20:36]               # y again: found at its first byte
    b = base.copy()
    b[200:216] = b[10:26]               # x again: the entry is y's, found one byte late
    wa = check(gpu_ctx, torch, a, 4096, "greater")
    wb = check(gpu_ctx, torch, b, 4096, "smaller")
    assert wa["matches"] == wb["matches"] == 1 and wa["match_bytes"] == wb["match_bytes"] + 1
    # the same with the two in the other order: now x's repeat is the one found
    c = rng.integers(0, 256, 400, dtype=np.uint8)
    put32(c, 10, y)
    put32(c, 20, x)
    c[200:216] = c[20:36]
    assert check(gpu_ctx, torch, c, 4096, "swapped")["match_bytes"] == wa["match_bytes"]


def test_match_against_the_block_end(S, torch, gpu_ctx):
    rng = np.random.default_rng(502)
    r = rng.integers(0, 256, 100, dtype=np.uint8)
    w = check(gpu_ctx, torch, np.concatenate([r, r]), 4096, "two halves")   # would run into the last five bytes
    assert (w["matches"], w["match_bytes"]) == (1, 95)
    n = 200
    for back, found in ((12, 1), (11, 0)):          # the last match start is n - 12
        a = rng.integers(0, 256, n, dtype=np.uint8)
        a[n - back:] = a[:back]
        a[n - back - 1] = a[n - back - 1] ^ 0xFF if back == 11 else a[n - back - 1]
        w = check(gpu_ctx, torch, a, 4096, back)
        assert w["matches"] == found, back


@pytest.mark.parametrize("period", [1, 2, 3, 7])
def test_overlapping_match(S, torch, gpu_ctx, period):
    rng = np.random.default_rng(503 + period)
    pat = rng.permutation(256)[:period].astype(np.uint8)
    a = np.concatenate([rng.integers(0, 256, 70, dtype=np.uint8), np.tile(pat, 1000 // period)])
    w = check(gpu_ctx, torch, a, 4096, period)
    assert w["match_bytes"] > 800


LENGTHS = [14, 15, 269, 270, 524, 525]


def test_every_length_step(S, torch, gpu_ctx):
    """Literal runs of 14, 15, 269, 270, 524 and 525 bytes lie on both sides of every step of
    ext(lit).  The match lengths are the same six numbers, and those straddle no step of
    ext(L - 4), which steps at L = 18 / 19, 273 / 274 and 528 / 529: test_every_match_length
    holds those."""
    rng = np.random.default_rng(504)
    for x in LENGTHS:
        # a source, a first match, then x literals (a stop byte and x - 1 more) and a match of x;
        # a colliding position can displace a start, so the seed is the first that parses as meant
        for seed in range(64):
            r = np.random.default_rng(5040 + 64 * x + seed)
            src = r.integers(0, 256, max(x + 40, 80), dtype=np.uint8)
            a = np.concatenate([src, src[:20], [src[20] ^ 0xFF], r.integers(0, 256, x - 1, dtype=np.uint8),
                                src[30:30 + x], [src[30 + x] ^ 0xFF], r.integers(0, 256, 20, dtype=np.uint8)])
            a = a.astype(np.uint8)
            seqs = R.parse_block(a).seqs
            if len(seqs) == 3 and seqs[1][0] == x and seqs[1][2] == x:
                break
        else:
            raise AssertionError(f"no block with a literal run and a match of {x}")
        check(gpu_ctx, torch, a, 4096, ("steps", x))
    for x in LENGTHS:                    # literal runs of exactly x, ended by a run of zeros
        b = np.concatenate([rng.integers(1, 256, x, dtype=np.uint8), np.zeros(40, np.uint8)])
        p = R.parse_block(b)
        assert p.seqs[0][0] == x + 1     # the first zero is a literal: the match starts at the second
        check(gpu_ctx, torch, b, 4096, x)
        b = np.concatenate([rng.integers(1, 256, x - 1, dtype=np.uint8), np.zeros(40, np.uint8)])
        assert R.parse_block(b).seqs[0][0] == x
        check(gpu_ctx, torch, b, 4096, -x)


def test_positions_inside_a_match_are_entered(S, torch, gpu_ctx):
    """A match over many whole groups; behind it a repeat of four bytes whose table entry was
    last written from inside the match (an earlier colliding position displaced the first one)."""
    for seed in range(64):       # the first seed whose starts no colliding position displaces
        rng = np.random.default_rng(5050 + seed)
        x, y = same_hash_pair(rng)
        a = rng.integers(0, 256, 1000, dtype=np.uint8)
        put32(a, 500, x)
        put32(a, 950, y)                             # displaces 500; not part of the copy below
        tail = np.concatenate([a[500:540], rng.integers(0, 256, 30, dtype=np.uint8)])
        block = np.concatenate([a, a[:900], np.array([a[900] ^ 0xFF], np.uint8), tail])
        seqs = R.parse_block(block).seqs
        # one match over 14 whole groups, then the repeat found at 1500, inside it
        if seqs[0] == (1000, 1000, 900) and seqs[1][:2] == (1, 1901 - 1500) and seqs[1][2] >= 35:
            break
    else:
        raise AssertionError("no such block")
    # were 1500 not entered, the entry would be y's at 950 and the repeat would start a byte late
    check(gpu_ctx, torch, block, 4096, "inside")


def test_size_equal_to_length(S, torch, gpu_ctx):
    """A block of 30 bytes with one match of four (a run of five): size == n, stored raw."""
    rng = np.random.default_rng(506)
    for run, delta in ((5, 0), (6, -1), (4, 2)):
        a = (np.arange(30) * 7 + 1).astype(np.uint8)
        a[11:11 + run] = 0xC3
        p = R.parse_block(a)
        assert p.size == 30 + delta
        pad = np.concatenate([a, rng.integers(0, 256, 18, dtype=np.uint8)])
        got = R.as_dict(gpu_ctx.measure_lz(dev(torch, pad), 30, block_bytes=4096))
        assert got == want_of([a], 4096)
        assert got["raw_blocks"] == (1 if delta >= 0 else 0) and got["stored_bytes"] == min(30, 30 + delta)


# ---- 4. streams ----------------------------------------------------------------------------

def strided(objs, stride, poison, lead=0):
    """The objects at a stride behind `lead` bytes, every gap (the one after the last object too)
    and the lead filled with poison."""
    buf = np.empty(lead + stride * len(objs), np.uint8)
    buf[:lead] = poison
    for j, a in enumerate(objs):
        lo = lead + j * stride
        buf[lo:lo + a.size] = a
        buf[lo + a.size:lo + stride] = (poison + 37 * j) & 0xFF
    return buf


def low_entropy_objs(rng, n, size):
    return [np.concatenate([rng.integers(0, 4, size // 2, dtype=np.uint8),
                            rng.integers(0, 256, size - size // 2, dtype=np.uint8)]) for _ in range(n)]


@pytest.mark.parametrize("bb", [4096, 8192, 65536])
def test_ragged_stream_ignores_gaps(S, torch, gpu_ctx, bb):
    rng = np.random.default_rng(600)
    size, stride = 12288 + 100, 12288 + 100 + 4096 + 12
    objs = low_entropy_objs(rng, 5, size)
    want = want_of(objs, bb)
    for lead, p in ((0, 0x00), (16, 0xA5), (4096 + 16, 0x03)):
        t = dev(torch, strided(objs, stride, p, lead))
        got = gpu_ctx.measure_lz_stream(t[lead:], size, 5, stride, block_bytes=bb)
        assert R.as_dict(got) == want, (lead, p)
    assert want["bytes"] == 5 * size


def test_identical_objects_behind_different_gaps(S, torch, gpu_ctx):
    rng = np.random.default_rng(601)
    a = low_entropy_objs(rng, 1, 8192 + 1)[0]         # the last block has one byte
    one = want_of([a], 4096)
    assert one["blocks"] == 3 and one["raw_blocks"] >= 1
    for stride in (8192 + 16, 8192 + 4096 + 32):      # object starts that are no multiple of 4096
        got = gpu_ctx.measure_lz_stream(dev(torch, strided([a] * 7, stride, 0x77)), a.size, 7, stride,
                                        block_bytes=4096)
        assert R.as_dict(got) == {k: 7 * v for k, v in one.items()}, stride


def test_stream_of_many_objects(S, torch, gpu_ctx):
    """65 538 objects of 100 bytes: more than one launch dimension holds."""
    n = 65535 + 3
    rng = np.random.default_rng(602)
    table = rng.integers(0, 3, (500, 100), dtype=np.uint8)
    table[17] = 0
    per = [want_of([row], 4096) for row in table]
    idx = np.arange(n) % 500
    idx[-3:] = (17, 1, 499)
    stride = 112
    buf = np.full((n, stride), 0xEE, np.uint8)
    buf[:, :100] = table[idx]
    counts = np.bincount(idx, minlength=500)
    want = {k: int(sum(int(c) * p[k] for c, p in zip(counts, per))) for k in R.FIELDS}
    got = gpu_ctx.measure_lz_stream(dev(torch, buf.reshape(-1)), 100, n, stride, block_bytes=4096)
    assert R.as_dict(got) == want
    assert got.blocks == n and got.bytes == 100 * n


def test_object_of_more_than_2_22_blocks(S, torch, gpu_ctx):
    """One zeroed object of 2^22 + 2 blocks of 4 KiB (above 16 GiB, offsets above 2^32) with
    three marker bytes, judged by closed form: a zero block is one match; a marker in the middle
    of a block splits it; the 100-byte tail is a block too.  The restatement runs on those three
    kinds of block only."""
    nb = (1 << 22) + 1
    n = nb * BLK + 100
    t = torch.zeros(n + 12, dtype=torch.uint8, device="cuda:0")
    marks = (5 * BLK + 1000, (1 << 32) + 3 * BLK + 1000, (nb - 1) * BLK + 1000)
    for pos in marks:
        t[pos] = 7
    zero = want_of([np.zeros(BLK, np.uint8)], BLK)
    m = np.zeros(BLK, np.uint8)
    m[1000] = 7
    marked = want_of([m], BLK)
    tail = want_of([np.zeros(100, np.uint8)], BLK)
    assert zero["matches"] == 1 and marked["matches"] > 1 and marked["literal_bytes"] == zero["literal_bytes"] + 1
    want = {k: (nb - 3) * zero[k] + 3 * marked[k] + tail[k] for k in R.FIELDS}
    got = gpu_ctx.measure_lz(t, n, block_bytes=BLK)
    assert R.as_dict(got) == want
    assert (got.bytes, got.blocks) == (n, nb + 1)
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("bb", [4096, 65536])
def test_stride_above_4_gib(S, torch, gpu_ctx, bb):
    """Two objects at a stride above 4 GiB; the gap is never initialised."""
    stride, size = (1 << 32) + 4096, 2 * 4096 + 1003
    rng = np.random.default_rng(603)
    a, b = low_entropy_objs(rng, 2, size)
    b[:3000] = a[:3000]
    t = torch.empty(stride + size + 13, dtype=torch.uint8, device="cuda:0")
    t[:size] = dev(torch, a)
    t[stride:stride + size] = dev(torch, b)
    want = want_of([a, b], bb)
    assert want != {k: 2 * v for k, v in want_of([a], bb).items()}   # the second object is not the first again
    got = gpu_ctx.measure_lz_stream(t, size, 2, stride, block_bytes=bb)
    assert R.as_dict(got) == want
    del t
    torch.cuda.empty_cache()


# ---- 5. accumulation ----------------------------------------------------------------------------

def test_adds_reuse_one_buffer(S, torch, gpu_ctx):
    """Three adds over one device buffer that fills on the same stream overwrite, no sync between;
    then the same again: twice everything."""
    size, n, stride = 8292, 4, 8304
    seeds = (1000, 2000, 3000)
    t = torch.zeros(stride * n, dtype=torch.uint8, device="cuda:0")
    objs = []
    for sb in seeds:
        gpu_ctx.fill_stream(t, size, n, stride, dedup=2, compress=2, seed_base=sb)
        torch.cuda.synchronize()
        h = host(t).copy()
        objs += [h[j * stride:j * stride + size] for j in range(n)]
    want = want_of(objs, BLK)
    st = torch.cuda.Stream()
    with gpu_ctx.lz_measurer(BLK) as m:
        for sb in seeds:
            gpu_ctx.fill_stream(t, size, n, stride, dedup=2, compress=2, seed_base=sb, stream=st)
            m.add_stream(t, size, n, stride, stream=st)
        assert R.as_dict(m.result()) == want
        for sb in seeds:
            gpu_ctx.fill_stream(t, size, n, stride, dedup=2, compress=2, seed_base=sb, stream=st)
            m.add_stream(t, size, n, stride, stream=st)
        assert R.as_dict(m.result()) == {k: 2 * v for k, v in want.items()}
    st.synchronize()


@pytest.mark.parametrize("bb", [4096, 12288, 65536])
def test_ranges_equal_the_whole(S, torch, gpu_ctx, bb):
    size = 5 * 65536 + 4097
    t = torch.zeros(size + 15, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.fill_controlled(t, size, dedup=3, compress=2, entropy=9)
    torch.cuda.synchronize()
    want = want_of([host(t, size)], bb)
    nb = -(-size // bb)
    cuts = [0, nb // 7, nb // 7 + 1, nb // 2, nb + 5]
    with gpu_ctx.lz_measurer(bb) as m:
        for lo, hi in zip(cuts, cuts[1:]):
            m.add_range(t[lo * bb:], size, lo, hi)
        m.add_range(t, size, 3, 3)             # empty ranges add nothing
        m.add_range(t, size, nb, nb + 1)
        assert R.as_dict(m.result()) == want
    assert R.as_dict(gpu_ctx.measure_lz(t, size, block_bytes=bb)) == want


def test_two_streams_two_threads(S, torch, gpu_ctx):
    rng = np.random.default_rng(700)
    parts = [low_entropy_objs(rng, 1, 64 * 4096 + 100)[0], low_entropy_objs(rng, 1, 3 * 65536 + 4097)[0]]
    ts = [dev(torch, p) for p in parts]
    torch.cuda.synchronize()               # the uploads ran on the default stream
    errs = []
    with gpu_ctx.lz_measurer(BLK) as m:
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
    want = want_of(parts, BLK)
    assert R.as_dict(r) == {k: 4 * v for k, v in want.items()}


def test_result_is_not_destructive(S, torch, gpu_ctx):
    rng = np.random.default_rng(701)
    a, b = low_entropy_objs(rng, 2, 20000)
    with gpu_ctx.lz_measurer(8192) as m:
        assert m.result() == S.LzResult()
        m.add(dev(torch, a))
        r1 = m.result()
        assert R.as_dict(r1) == want_of([a], 8192) and m.result() == r1
        m.add(dev(torch, b))
        assert R.as_dict(m.result()) == want_of([a, b], 8192)
        m.reset()
        assert m.result() == S.LzResult()
        m.add(dev(torch, b))
        assert R.as_dict(m.result()) == want_of([b], 8192)
    with gpu_ctx.lz_measurer() as m:
        assert m.block_bytes == 65536
        m.add_stream(0, 0, 5)                  # zero-length adds launch nothing, whatever the pointer
        m.add_stream(0, 4096, 0)
        assert m.result() == S.LzResult()


# ---- 6. host buffers ---------------------------------------------------------------------------

def test_measure_lz_data_buffers(S):
    rng = np.random.default_rng(800)
    a = low_entropy_objs(rng, 1, 64 * 4096 + 100)[0]
    for bb in (4096, 65536):
        want = want_of([a], bb)
        assert R.as_dict(S.measure_lz_data(bytearray(a.tobytes()), bb)) == want
        assert R.as_dict(S.measure_lz_data(a.tobytes(), bb)) == want                  # read-only bytes
        shifted = np.empty(a.size + 1, np.uint8)
        shifted[1:] = a
        assert R.as_dict(S.measure_lz_data(shifted[1:], bb)) == want                  # a view at offset 1
    assert R.as_dict(S.measure_lz_data(a)) == want_of([a], 65536)
    assert S.measure_lz_data(b"") == S.LzResult()


@functools.lru_cache(maxsize=None)
def tiled_block_results(bb):
    """Eight distinct 12288-byte blocks and their results: the buffers of the chunk-edge test are
    built from them, so the restatement runs on eight blocks, not on 64 MiB."""
    rng = np.random.default_rng(801)
    blocks = [np.concatenate([rng.integers(0, 3, bb // 2, dtype=np.uint8),
                              rng.integers(0, 256, bb - bb // 2, dtype=np.uint8)]) for _ in range(8)]
    return blocks, [want_of([b], bb) for b in blocks]


@pytest.mark.parametrize("over", [-1, 0, 1, 2])
def test_measure_lz_data_across_the_chunk_edge(S, over):
    """12288-byte blocks: a chunk is 5461 whole blocks (67 104 768 bytes, not 64 MiB); buffers
    that end a block before, at and behind the chunk's edge, with a ragged tail."""
    bb = 12288
    per = HOST_CHUNK // bb
    assert (per, per * bb) == (5461, 67104768)
    blocks, results = tiled_block_results(bb)
    nb = per + over
    idx = (np.arange(nb) * 5 + 3) % 8
    tail = blocks[2][:100]
    a = np.concatenate([np.stack(blocks)[idx].reshape(-1), tail])
    tw = want_of([tail], bb)
    counts = np.bincount(idx, minlength=8)
    want = {k: int(sum(int(c) * r[k] for c, r in zip(counts, results))) + tw[k] for k in R.FIELDS}
    got = S.measure_lz_data(a, block_bytes=bb)
    assert R.as_dict(got) == want
    assert got.blocks == nb + 1


# ---- 7. refusals on the device ---------------------------------------------------------------------

def test_refusals(S, torch, gpu_ctx):
    t = torch.zeros(3 * 8192, dtype=torch.uint8, device="cuda:0")
    with gpu_ctx.lz_measurer(BLK) as m:
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
        assert m.result() == S.LzResult()
    for bb in (0, 4095, 8191, 69632, 131072):
        with pytest.raises(ValueError, match="block_bytes must be a multiple of 4096 from 4096 to 65536"):
            gpu_ctx.lz_measurer(bb)


# ---- 8. every match length ---------------------------------------------------------------------------

def sweep(ctx, torch, cases, bb=BLK):
    """Crafted blocks of one size as one strided stream with poisoned gaps, one call; the sum
    against the restatement's.  Only a wrong sum measures them one by one, to name the first."""
    size = cases[0].block.size
    assert all(c.block.size == size for c in cases) and size <= bb
    stride = size + -size % 16 + 16
    buf = strided([c.block for c in cases], stride, 0xEE)
    got = R.as_dict(ctx.measure_lz_stream(dev(torch, buf), size, len(cases), stride, block_bytes=bb))
    want = K.total(cases)
    assert want["blocks"] == len(cases) and want["matches"] >= len(cases)
    if got != want:
        for c in cases:
            one = R.as_dict(ctx.measure_lz(dev(torch, c.block), size, block_bytes=bb))
            assert one == K.result(c.parse), f"first wrong case: {c.name}, match {c.triple}"
        raise AssertionError(f"every case alone is right, the stream's sum is not: {got} != {want}")
    return want


def test_every_match_length(S, torch, gpu_ctx):
    """L = 4..1030 ended by a differing byte: every (step, lane, count) at which the extension
    loop can end in steps 0 to 2, and step 4; both sides of ext(L - 4)'s steps at 18 / 19,
    273 / 274 and 528 / 529."""
    cases = K.mismatch_sweep()
    lengths = [c.triple[2] for c in cases]
    assert lengths == list(range(4, 1031))
    assert {18, 19, 273, 274, 528, 529, 256, 512, 768, 1024} <= set(lengths)
    for c in cases[::97]:        # the judge itself, on a few: the cached parse is the restatement's
        assert K.result(c.parse) == want_of([c.block], BLK)
    sweep(gpu_ctx, torch, cases)


def test_every_match_length_to_the_block_end(S, torch, gpu_ctx):
    """L = 7..1030 with the copy equal through the block's last byte: the clamp at maxL in every
    lane and count, and at maxL = 256, 512, 768 and 1024 the exit that flags no lane."""
    cases = K.block_end_sweep()
    assert [c.triple[2] for c in cases] == list(range(7, 1031))
    for c in cases:
        start, off, L = c.triple
        assert start + L == c.block.size - 5 and c.block[-1] == c.block[-1 - off]
    sweep(gpu_ctx, torch, cases)


def test_match_ended_among_the_last_five_bytes(S, torch, gpu_ctx):
    """The copy goes on for 0 to 4 bytes behind n - 5 and then differs: the extension's last
    lane holds equal bytes past maxL, which must not count, at every place of its dword."""
    cases = K.last_five_sweep()
    assert len(cases) == 710
    assert all(c.triple[0] + c.triple[2] == c.block.size - 5 for c in cases)
    sweep(gpu_ctx, torch, cases)


def test_short_matches_at_every_alignment(S, torch, gpu_ctx):
    """L = 4..40 at all 16 pairs of (match start mod 4, source mod 4): both funnel shifts."""
    cases = K.dense_sweep()
    assert len({(c.triple[2], c.triple[0] % 4, (c.triple[0] - c.triple[1]) % 4) for c in cases}) == 37 * 16
    sweep(gpu_ctx, torch, cases)


# ---- 9. offsets ------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(13))
def test_far_match(S, torch, gpu_ctx, k):
    """Offsets up to the greatest there is (65 524: source at 0, match at n - 12 of a 65 536-byte
    block), sources at 2^15 - 2 .. 2^15 and above, far matches of 256, 257, 4000 and 4096 bytes."""
    cases = K.far_cases()
    assert len(cases) == 13
    c = cases[k]
    assert c.triple in K.triples(c.parse), c.name        # the far match is in the parse
    if k < 2:
        assert c.triple == (c.block.size - 12, c.block.size - 12, 7)
    want = check(gpu_ctx, torch, c.block, 65536, c.name)
    assert want == K.result(c.parse)


# ---- 10. the table -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 5, 16])
def test_same_hash_group(S, torch, gpu_ctx, k):
    """k words of one hash in one group: the last one's repeat is found at its first byte, every
    other one's a byte late."""
    cases = K.table_cases()["groups"][k]
    wants = [check(gpu_ctx, torch, c.block, BLK, c.name) for c in cases]
    assert all(w["matches"] == 1 for w in wants)
    assert [w["match_bytes"] for w in wants] == [wants[-1]["match_bytes"] - 1] * (k - 1) + [K.TABLE_L]


def test_chained_hash_pair(S, torch, gpu_ctx):
    """Two overlapping words of one hash: the first leaves its entry to the second inside a
    group, and enters itself at lane 63."""
    inside, edge_later, edge_same = K.table_cases()["chained"]
    wants = [check(gpu_ctx, torch, c.block, BLK, c.name) for c in (inside, edge_later, edge_same)]
    assert [w["matches"] for w in wants] == [1, 1, 1]
    assert [c.triple[2] for c in (inside, edge_later, edge_same)] == [15, 15, 8]      # late, late, at once
    assert [w["match_bytes"] for w in wants] == [15, 15, 8]


def test_source_at_every_lane(S, torch, gpu_ctx):
    cases = K.source_at_every_lane()
    found = [c for c in cases if c.triple in K.triples(c.parse)]
    assert len(found) == 128 and [c.triple[0] - c.triple[1] for c in found] == list(range(128))
    sweep(gpu_ctx, torch, cases)
    for q in (0, 1, 62, 63, 64, 127):        # and alone, so a wrong one has a name
        check(gpu_ctx, torch, cases[q].block, BLK, q)


# ---- 11. a wave's later blocks -------------------------------------------------------------------------

def reuse_objects(bb):
    """Seven distinct objects of two full blocks and a ragged one, every block half bytes of 4
    values and half random."""
    rng = np.random.default_rng(900 + bb)
    return [np.concatenate(low_entropy_objs(rng, 2, bb) + low_entropy_objs(rng, 1, 1000)) for _ in range(7)]


@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_wave_takes_later_blocks(S, torch, gpu_ctx, bb):
    """More than three blocks for every wave of the grid, its successive blocks of different
    content and length: the table clear and the staging over the previous block's LDS."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * min(32, (160 << 10) // (bb + (8 << 10)))
    size = 2 * bb + 1000
    n_objs = grid + 7
    blocks = 3 * n_objs
    assert blocks > 3 * grid
    # block i is block i % 3 of object i // 3, a copy of object (i // 3) % 7
    i = np.arange(blocks)
    content = (i // 3) % 7 * 3 + i % 3
    ragged = i % 3 == 2
    assert (content[:-grid] != content[grid:]).all()              # blocks w and w + grid, every w
    assert (~ragged[:-grid] & ragged[grid:]).any() and (ragged[:-grid] & ~ragged[grid:]).any()
    objs = reuse_objects(bb)
    distinct = {o[lo:lo + bb].tobytes() for o in objs for lo in range(0, size, bb)}
    assert len(distinct) == 21 and all(o.size == size for o in objs)
    per = [want_of([o], bb) for o in objs]
    assert all(p["blocks"] == 3 and p["matches"] > 100 for p in per)
    counts = np.bincount(np.arange(n_objs) % 7, minlength=7)
    want = {k: int(sum(int(c) * p[k] for c, p in zip(counts, per))) for k in R.FIELDS}
    stride = size + -size % 16 + 16
    buf = strided([objs[j % 7] for j in range(n_objs)], stride, 0x3C)
    got = gpu_ctx.measure_lz_stream(dev(torch, buf), size, n_objs, stride, block_bytes=bb)
    assert R.as_dict(got) == want
    assert got.blocks == blocks
