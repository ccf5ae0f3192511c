"""GPU: a payload's dedup under content-defined chunking (k_chunk_candidates,
k_chunk_cuts, k_chunk_fp, the distinct count and the surfaces over them;
DESIGN.md §5.11).

The judge is a numpy restatement of the definition, written from the document
in tests/chunk_restatement.py: G, the 32-byte window sums (vectorised), the cut rule (a Python loop
over the cuts), and `bytes` of every chunk in a dict for the distinct counts,
never a restatement of the fingerprint.  Every field is compared exactly.
"""
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MiB = 1 << 20
DEFAULTS = (2048, 8192, 65536)
SMALL = (32, 64, 256)
PARAMS = [SMALL, (64, 256, 1024), (100, 128, 1000), DEFAULTS]
SIZES = [1, 31, 32, 33, 63, 64, 255, 256, 257, 4095, 4096, 4097, 65613, MiB + 5]
EVENTS = {"cut_at_min", "skipped_before_min", "candidate_at_max", "forced", "forced_then_candidate"}


# ---- the definition, restated (tests/chunk_restatement.py) -----------------------

from chunk_restatement import G, _gear, candidates, cuts_of, restate, window_hash  # noqa: E402,F401


# ---- fixtures -----------------------------------------------------------------------

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


def strided(objs, stride, poison):
    """The objects at a stride, the gaps (and the space after the last one) filled with `poison`."""
    buf = np.full(stride * len(objs), poison, np.uint8)
    for j, o in enumerate(objs):
        buf[j * stride:j * stride + len(o)] = o
    return buf


@functools.lru_cache(maxsize=None)
def random_bytes(size, seed=1):
    a = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def window13():
    """A 32-byte string whose window hash passes at bits = 13 (found by search on the CPU)."""
    rng = np.random.default_rng(13)
    while True:
        rows = rng.integers(1, 256, (1 << 16, 32), dtype=np.uint8)
        hit = np.flatnonzero((window_hash(rows)[:, 0] >> np.uint32(19)) == 0)
        if hit.size:
            w = rows[hit[0]].copy()
            w.setflags(write=False)
            return w


def zeros_with(size, ends, w):
    """Zeros with the string w placed so that it ends at each offset of `ends` (its
    head cut off where it would start before the object)."""
    a = np.zeros(size, np.uint8)
    for e in ends:
        lo = e - 31
        a[max(lo, 0):e + 1] = w[max(-lo, 0):]
    return a


# ---- 1. random bytes --------------------------------------------------------------------

@pytest.mark.parametrize("params", PARAMS, ids=str)
def test_random_bytes(S, torch, gpu_ctx, params):
    events = set()
    for size in SIZES:
        a = random_bytes(size)
        t = dev(torch, np.concatenate([a, np.full(16, 0xEE, np.uint8)]))
        got = gpu_ctx.measure_chunks(t, size, *params)
        want = restate(S, [a], params, events)
        assert got == want, size
        assert got.unique_bytes == size                     # random chunks of >= 32 bytes never repeat
    if params == SMALL:
        assert events == EVENTS, EVENTS - events            # every event of the cut rule was met


def test_gear_table_or_arithmetic(S, torch, gpu_ctx):
    """The candidate pass with G from LDS and with G computed: the same result."""
    a = random_bytes(MiB + 5)
    t = dev(torch, a)
    want = restate(S, [a], SMALL)
    for table in (True, False):
        with gpu_ctx.chunker(*SMALL) as h:
            h.gear_table(table)
            h.add(t)
            assert h.result() == want, table


# ---- 2. crafted windows -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_objects():
    """(ends, objects, size, stride): the window ends at every offset from 4064 to
    4128 of a zero background, one object each."""
    w = window13()
    size, stride = 3 * 4096 + 77, 3 * 4096 + 96
    ends = list(range(4064, 4129))
    objs = [zeros_with(size, [e], w) for e in ends]
    for o in objs:
        o.setflags(write=False)
    return ends, objs, size, stride


def chunked(ctx, table, params, add):
    """The result of one handle, G from LDS (table) or computed, after add(handle)."""
    with ctx.chunker(*params) as h:
        h.gear_table(table)
        add(h)
        return h.result()


def test_window_at_every_granule_and_lane_edge(S, torch, gpu_ctx):
    """The window ends at every offset from 4064 to 4128 of a zero background: the
    granule's edge, both sides of it, and every lane-run edge near it; with G
    from LDS and with G computed."""
    ends, objs, size, stride = edge_objects()
    buf, want = dev(torch, strided(objs, stride, 0x5A)), restate(S, objs, DEFAULTS)
    ones = [(e, dev(torch, np.concatenate([o, np.full(19, 0x5A, np.uint8)])), restate(S, [o], DEFAULTS))
            for e, o in zip(ends, objs)]
    for table in (True, False):
        got = chunked(gpu_ctx, table, DEFAULTS, lambda h: h.add_stream(buf, size, len(objs), stride))
        assert got == want, table
        for e, t, w1 in ones:                              # one by one: a miss names its offset
            r = chunked(gpu_ctx, table, DEFAULTS, lambda h: h.add(t, size))
            assert r == w1, (table, e)
            assert r.candidates >= 1 and r.chunks == 2 and r.forced_cuts == 0


def test_window_edges_in_a_batch_with_g_computed(S, torch, gpu_ctx):
    """The same 65 objects as one batch add, G computed per byte."""
    ends, objs, size, stride = edge_objects()
    buf = dev(torch, strided(objs, stride, 0x5A))
    spans = [(j * stride, size) for j in range(len(objs))]
    assert chunked(gpu_ctx, False, DEFAULTS, lambda h: h.add_batch(buf, spans)) == restate(S, objs, DEFAULTS)


@pytest.mark.parametrize("mn,mx,first", [(2048, 65536, 5000), (2048, 65536, None), (32, 256, None), (100, 1000, 777)],
                         ids=str)
def test_window_against_min_and_max(S, torch, gpu_ctx, mn, mx, first):
    """The window ends at s + min - 2, s + min - 1, s + max - 1 and s + max, s the
    start of the object or the byte after an earlier cut at `first`.  With min = 32
    at the object's start these are offsets 30 and 31: one byte before the first
    possible candidate, where the string is none, and the first possible candidate."""
    w = window13()
    params = (mn, 8192, mx)
    s = 0 if first is None else first + 1
    size = s + mx + 2 * mn + 77
    objs = []
    for d in (mn - 2, mn - 1, mx - 1, mx):
        objs.append(zeros_with(size, ([] if first is None else [first]) + [s + d], w))
    events = set()
    want = [restate(S, [o], params, events) for o in objs]
    for o, r in zip(objs, want):
        got = gpu_ctx.measure_chunks(dev(torch, np.concatenate([o, np.full(16, 0xC3, np.uint8)])), size, *params)
        assert got == r
    assert events == EVENTS - ({"skipped_before_min"} if s + mn - 2 < 31 else set())


# ---- 3. constant objects -------------------------------------------------------------------

@pytest.mark.parametrize("params,size", [((100, 128, 1000), 12345), (DEFAULTS, 300001), (SMALL, 4097)], ids=str)
def test_zeros_are_forced_cuts_only(S, torch, gpu_ctx, params, size):
    z = np.zeros(size, np.uint8)
    got = gpu_ctx.measure_chunks(dev(torch, z), size, *params)
    assert got == restate(S, [z], params)
    mx = params[2]
    assert got == S.ChunkResult(size, size // mx + 1, 2, mx + size % mx, 0, size // mx)


@pytest.mark.parametrize("mn,mx,size", [(100, 1000, 12345), (32, 256, 8191), (37, 37, 5000)], ids=str)
def test_constant_candidate_byte_cuts_every_min(S, torch, gpu_ctx, mn, mx, size):
    """Byte 57 is a candidate everywhere at bits = 6; byte 0 is not."""
    a = np.full(size, 57, np.uint8)
    got = gpu_ctx.measure_chunks(dev(torch, a), size, mn, 64, mx)
    assert got == restate(S, [a], (mn, 64, mx))
    assert got == S.ChunkResult(size, -(-size // mn), 2, mn + size % mn, size - 31, 0)
    z = np.zeros(size, np.uint8)
    assert gpu_ctx.measure_chunks(dev(torch, z), size, mn, 64, mx).candidates == 0


# ---- 4. fixed blocks ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def generated(S, torch, gpu_ctx):
    """Payloads filled on the GPU (device tensor, host copy), made once."""
    @functools.lru_cache(maxsize=None)
    def get(kind, size, dedup, compress):
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda:0")
        t[size:] = 0xEE
        if kind == "controlled":
            gpu_ctx.fill_controlled(t, size, dedup=dedup, compress=compress, entropy=42)
        elif kind == "dgen":
            gpu_ctx.dgen_fill(t, size, dedup=dedup, compress=compress, seed=7)
        else:
            t[:size] = torch.from_numpy(np.array(random_bytes(size, 9))).to("cuda:0")
        torch.cuda.synchronize()
        a = t[:size].cpu().numpy()
        a.setflags(write=False)
        return t, a
    return get


@pytest.mark.parametrize("block", [4096, 12288])
@pytest.mark.parametrize("kind,size,dedup,compress", [("random", 3 * MiB + 4097, 0, 0), ("controlled", 3 * MiB + 4097, 1, 1),
                                                      ("controlled", 3 * MiB + 4097, 4, 2), ("dgen", 2 * MiB, 3, 2)],
                         ids=str)
def test_min_equal_max_is_fixed_blocks(S, torch, gpu_ctx, generated, block, kind, size, dedup, compress):
    t, a = generated(kind, size, dedup, compress)
    got = gpu_ctx.measure_chunks(t, size, block, 8192, block)
    m = gpu_ctx.measure(t, size, block_bytes=block)
    assert (got.chunks, got.unique_chunks, got.bytes) == (m.blocks, m.unique_blocks, m.bytes)
    blocks = {bytes(a[o:o + block]) for o in range(0, size, block)}
    assert got.unique_chunks == len(blocks) and got.unique_bytes == sum(len(b) for b in blocks)


# ---- 5. generated payloads --------------------------------------------------------------------

@pytest.mark.parametrize("params", [DEFAULTS, SMALL], ids=str)
@pytest.mark.parametrize("kind,dedup,compress", [("controlled", d, c) for d in (1, 2, 4) for c in (1, 2, (3, 2))] +
                         [("dgen", 3, 2)], ids=str)
def test_generated_payloads(S, torch, gpu_ctx, generated, kind, dedup, compress, params):
    size = 2 * MiB if kind == "dgen" else MiB + 4097
    t, a = generated(kind, size, dedup, compress)
    assert gpu_ctx.measure_chunks(t, size, *params) == restate(S, [a], params)


# ---- 6. streams ---------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [SMALL, DEFAULTS], ids=str)
def test_ragged_stream_ignores_gaps(S, torch, gpu_ctx, params):
    rng = np.random.default_rng(5)
    size, stride = 70001, 70001 + 4096 + 15            # a 16-byte aligned stride with a > 4 KiB gap
    objs = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(5)]
    objs[3][:30000] = objs[1][:30000]                  # shared content between objects
    objs[4] = objs[0].copy()                           # two byte-identical objects behind different gaps
    want = restate(S, objs, params)
    gaps = strided(objs, stride, 0)
    gaps[size:stride] = 0x33                           # ... so that a window crossing into the object would differ
    gaps[3 * stride + size:4 * stride] = 0x77
    for buf in (strided(objs, stride, 0x00), strided(objs, stride, 0xA5), gaps):
        assert gpu_ctx.measure_chunks_stream(dev(torch, buf), size, 5, stride, *params) == want
    pair = gpu_ctx.measure_chunks_stream(dev(torch, strided([objs[0], objs[4]], stride, 0x99)), size, 2, stride,
                                         *params)
    assert pair.chunks == 2 * pair.unique_chunks and pair.bytes == 2 * pair.unique_bytes


def test_tiny_objects(S, torch, gpu_ctx):
    rng = np.random.default_rng(6)
    objs = [rng.integers(0, 256, 100, dtype=np.uint8) for _ in range(7)]
    objs[5] = objs[2].copy()
    buf = dev(torch, strided(objs, 112, 0x11))
    for table in (True, False):                            # G from LDS, G computed
        for v in (0, 57):
            b = np.full(1, v, np.uint8)
            t = dev(torch, np.concatenate([b, np.full(15, 0xEE, np.uint8)]))
            r = chunked(gpu_ctx, table, SMALL, lambda h: h.add(t, 1))
            assert r == restate(S, [b], SMALL) == S.ChunkResult(1, 1, 1, 1, 0, 0), (table, v)
        for params in (SMALL, DEFAULTS):
            r = chunked(gpu_ctx, table, params, lambda h: h.add_stream(buf, 100, 7, 112))
            assert r == restate(S, objs, params), (table, params)


def test_stream_across_object_split(S, torch, gpu_ctx):
    """More than 65 535 objects: pass A's launch is split along the objects."""
    n = 65535 + 3
    rows = np.random.default_rng(8).integers(0, 256, (n, 100), dtype=np.uint8)
    rows[-1] = rows[65534]                             # the objects on both sides of the split, repeated
    rows[-2] = rows[65535]
    buf = np.full((n, 112), 0x42, np.uint8)
    buf[:, :100] = rows
    r = gpu_ctx.measure_chunks_stream(dev(torch, buf.reshape(-1)), 100, n, 112, *SMALL)
    assert r == restate(S, list(rows), SMALL)
    assert r.bytes == 100 * n and r.unique_chunks < r.chunks


def test_stride_above_4_gib(S, torch, gpu_ctx):
    """Two small objects at a stride above 4 GiB; the gap is never initialised."""
    stride, size = (1 << 32) + 4096, 5003
    a = random_bytes(size, 21)
    b = a.copy()
    b[2500] ^= 1
    t = torch.empty(stride + size + 13, dtype=torch.uint8, device="cuda:0")
    t[:size] = dev(torch, a)
    t[stride:stride + size] = dev(torch, b)
    r = gpu_ctx.measure_chunks_stream(t, size, 2, stride, *SMALL)
    assert r == restate(S, [a, b], SMALL)
    assert r.chunks // 2 < r.unique_chunks < r.chunks    # only the chunks around byte 2500 differ
    del t
    torch.cuda.empty_cache()


def test_bytes_around_the_objects_are_not_read(S, torch, gpu_ctx):
    """The result does not change with the bytes before the buffer, in the gap and
    after the last object (whose end shares a 16-byte piece with them)."""
    size, stride, n, lead = 4096 + 1001, 4096 + 1008, 3, 4096
    objs = [random_bytes(size, 30 + j) for j in range(n)]
    want = restate(S, objs, SMALL)
    for poison in (0x00, 0xFF, 57):
        host = np.full(lead + n * stride + 4096, poison, np.uint8)
        for j, o in enumerate(objs):
            host[lead + j * stride:lead + j * stride + size] = o
        t = dev(torch, host)
        assert gpu_ctx.measure_chunks_stream(t[lead:], size, n, stride, *SMALL) == want, poison
        with gpu_ctx.chunker(100, 64, 1000) as h:        # bits = 6: byte 57 is a candidate wherever it is read
            h.add_stream(t[lead:], size, n, stride)
            assert h.result() == restate(S, objs, (100, 64, 1000)), poison


# ---- 7. shift -----------------------------------------------------------------------------------

def test_shifted_copy_deduplicates(S, torch, gpu_ctx):
    """B = one extra byte + A: content-defined cuts find A's chunks again, which
    fixed blocks cannot."""
    a = random_bytes(MiB, 40)
    b = np.concatenate([np.full(1, 0x5C, np.uint8), a])
    want = restate(S, [a, b], DEFAULTS)
    assert want.unique_bytes < 0.6 * (len(a) + len(b))
    with gpu_ctx.chunker() as h:
        h.add(dev(torch, a))
        h.add(dev(torch, np.concatenate([b, np.full(15, 0, np.uint8)])), len(b))
        got = h.result()
    assert got == want
    fixed = gpu_ctx.chunker(4096, 8192, 4096)
    fixed.add(dev(torch, a))
    fixed.add(dev(torch, np.concatenate([b, np.full(15, 0, np.uint8)])), len(b))
    assert fixed.result().unique_bytes == len(a) + len(b)
    fixed.close()


# ---- 8. pass C: a chunk at any shift, every byte of it in the fingerprint ---------------------------
# Parameters (32, 65536, M).  An object is s filler bytes, the string of window16()
# (the object's only candidate, so the first chunk is [0, 31 + s]) and K times M
# bytes that forced cuts close: chunk k starts at byte 32 + s + k M, at shift
# (s + k M) mod 16, and the last one ends with the object, unaligned for most s.
# The builders below need no GPU; tests/test_chunks_cpu.py checks through the
# restatement that the objects parse as meant.

FP_AVG = 65536
SHORT = tuple(range(48, 64))           # 3 or 4 pieces, every tail length 0..15
LONG = (2064, 2065, 2072, 2079)        # 129 or 130 pieces (three laps of a lane), tails 0, 1, 8, 15
SHIFTS = range(16)


@functools.lru_cache(maxsize=None)
def window16():
    """A 32-byte string whose window hash passes at bits = 16 (found by search on the CPU)."""
    rng = np.random.default_rng(16)
    while True:
        rows = rng.integers(1, 256, (1 << 16, 32), dtype=np.uint8)
        hit = np.flatnonzero((window_hash(rows)[:, 0] >> np.uint32(16)) == 0)
        if hit.size:
            w = rows[hit[0]].copy()
            w.setflags(write=False)
            return w


def only_w_candidate(obj, s):
    """The object's one candidate at bits = 16 is the end of the string placed behind s bytes."""
    return np.flatnonzero(candidates(obj, 16)[0]).tolist() == [31 + s]


def parsed_as_meant(rows, s, M, K=2):
    """How many of the equal-length objects are the chunks [0, 31 + s] and K forced cuts of M bytes."""
    meant = [(0, 31 + s)] + [(32 + s + k * M, 31 + s + (k + 1) * M) for k in range(K)]
    return sum(cuts_of(c, 32, M)[:2] == (meant, K) for c in candidates(rows, 16))


@functools.lru_cache(maxsize=None)
def shifted_base(s, M):
    """filler(s) | w | X0 | X1, X0 and X1 of M bytes: the first seed whose object has no
    candidate but w's end and whose X0 has no two equal chunk-relative 16-byte pieces
    (so that no exchange of two is a no-op)."""
    w = window16()
    attempt = 0
    while True:
        rng = np.random.default_rng([8, s, M, attempt])
        a = np.concatenate([rng.integers(0, 256, s, dtype=np.uint8), w, rng.integers(0, 256, 2 * M, dtype=np.uint8)])
        pieces = a[32 + s:32 + s + M // 16 * 16].reshape(-1, 16)
        if only_w_candidate(a, s) and len({bytes(p) for p in pieces}) == len(pieces):
            a.setflags(write=False)
            return a
        attempt += 1


def flip_set(M):
    """The bytes of a chunk that get a variant: all of a short one; pieces 0, 1, 63, 64, 65
    and the last two of a long one."""
    if M < 1024:
        return np.arange(M)
    P = (M + 15) // 16
    return np.array([q for p in (0, 1, 63, 64, 65, P - 2, P - 1) for q in range(16 * p, min(16 * p + 16, M))])


@functools.lru_cache(maxsize=None)
def every_byte_case(s, M):
    """The base, one copy per byte q of flip_set(M) with bit (q + s) % 8 of that byte of X0
    flipped, the same for X1, and the base again: one object per row."""
    a = shifted_base(s, M)
    qs = flip_set(M)
    out = np.tile(a, (2 * qs.size + 2, 1))
    bit = (1 << ((qs + s) % 8)).astype(np.uint8)
    for k in (0, 1):
        out[1 + k * qs.size + np.arange(qs.size), 32 + s + k * M + qs] ^= bit
    out.setflags(write=False)
    return out


def swap_pairs(M):
    """(p, q = p | 1 << b) over the whole pieces of a chunk of M bytes."""
    P = M // 16
    return [(p, p | (1 << b)) for p in range(P) for b in range(P.bit_length()) if not p >> b & 1 and p | (1 << b) < P]


@functools.lru_cache(maxsize=None)
def swap_case(s, M):
    """The base, one copy per pair of swap_pairs(M) with the chunk-relative pieces p and q
    of X0 exchanged (for s != 0 not 16-byte aligned in the object), and the base again."""
    a = shifted_base(s, M)
    o = 32 + s
    pairs = swap_pairs(M)
    out = np.tile(a, (len(pairs) + 2, 1))
    for i, (p, q) in enumerate(pairs, 1):
        out[i, o + 16 * p:o + 16 * p + 16] = a[o + 16 * q:o + 16 * q + 16]
        out[i, o + 16 * q:o + 16 * q + 16] = a[o + 16 * p:o + 16 * p + 16]
    out.setflags(write=False)
    return out


def strided_each(rows, stride):
    """strided() with a poison of its own (never zero) behind every object."""
    buf = np.empty((rows.shape[0], stride), np.uint8)
    buf[:] = (1 + 37 * np.arange(rows.shape[0]) % 255).astype(np.uint8)[:, None]
    buf[:, :rows.shape[1]] = rows
    return buf.reshape(-1)


def stream_of(torch, ctx, rows, params):
    n, size = rows.shape
    stride = (size + 15) // 16 * 16 + 16
    return ctx.measure_chunks_stream(dev(torch, strided_each(rows, stride)), size, n, stride, *params)


@pytest.mark.parametrize("M", SHORT + LONG)
def test_fp_every_byte(S, torch, gpu_ctx, M):
    """Every byte enters, at every shift and tail: a flipped bit anywhere in a chunk,
    mid-object or at the object's unaligned end, is a chunk of its own."""
    params = (32, FP_AVG, M)
    for s in SHIFTS:
        rows = every_byte_case(s, M)
        n = rows.shape[0]
        want = restate(S, list(rows), params)
        assert want.bytes == rows.size and want.chunks >= 3 * n and 3 + (n - 2) <= want.unique_chunks
        got = stream_of(torch, gpu_ctx, rows, params)
        assert got == want, (s, M)


# ---- 9. pass C: pieces are keyed by their index in the chunk ----------------------------------------

@pytest.mark.parametrize("M", LONG)
def test_fp_piece_swaps(S, torch, gpu_ctx, M):
    """Two pieces of a chunk whose indices differ in one bit, exchanged: a chunk of its own."""
    params = (32, FP_AVG, M)
    for s in SHIFTS:
        rows = swap_case(s, M)
        n = rows.shape[0]
        assert n - 2 == len(swap_pairs(M)) > 7 * 64
        assert len({bytes(r) for r in rows}) == n - 1     # numpy: every variant differs from the base and the others
        want = restate(S, list(rows), params)
        assert want.unique_chunks >= 3 + (n - 2)
        got = stream_of(torch, gpu_ctx, rows, params)
        assert got == want, (s, M)


# ---- 10. pass C: equal content is one fingerprint wherever it lies ----------------------------------

@functools.lru_cache(maxsize=None)
def everywhere_case(M):
    """For every s the object filler(s) | w | X | Y_s | X, one X for all: it lies mid-object
    and at the object's end, at every shift.  No candidate but w's end, the Y_s distinct."""
    w = window16()
    attempt = 0
    while True:
        rng = np.random.default_rng([10, M, attempt])
        X = rng.integers(0, 256, M, dtype=np.uint8)
        objs = [np.concatenate([rng.integers(0, 256, s, dtype=np.uint8), w, X, rng.integers(0, 256, M, dtype=np.uint8), X])
                for s in SHIFTS]
        mids = {bytes(o[32 + s + M:32 + s + 2 * M]) for s, o in enumerate(objs)} | {bytes(X)}
        if all(only_w_candidate(o, s) for s, o in enumerate(objs)) and len(mids) == 17:
            for o in objs:
                o.setflags(write=False)
            return tuple(objs)
        attempt += 1


@pytest.mark.parametrize("M", SHORT + LONG)
def test_fp_same_chunk_everywhere(S, torch, gpu_ctx, M):
    """A fingerprint that depended on the shift, on a byte past the chunk or on a byte past
    the object would count more than one X."""
    params = (32, FP_AVG, M)
    objs = everywhere_case(M)
    want = restate(S, objs, params)
    assert want == S.ChunkResult(sum(len(o) for o in objs), 64, 33, sum(32 + s for s in SHIFTS) + 17 * M, 16, 48)
    with gpu_ctx.chunker(*params) as h:
        for s, o in enumerate(objs):                       # sizes differ: an add each, its own poison behind it
            tail = np.full(16 + -len(o) % 16, 0x11 + 13 * s, np.uint8)
            h.add(dev(torch, np.concatenate([o, tail])), len(o))
        got = h.result()
    assert got == want


# ---- 11. pass C: length alone separates ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def length_case(t):
    """w | Z with Z of 60 bytes, the last t zero (closed by a forced cut at max = 60), and
    w | Z[:60 - t] (closed by the object's end): the same zero-padded pieces, the same
    piece count, another length."""
    w = window16()
    attempt = 0
    while True:
        Z = np.random.default_rng([11, t, attempt]).integers(1, 256, 60, dtype=np.uint8)
        Z[60 - t:] = 0
        a, b = np.concatenate([w, Z]), np.concatenate([w, Z[:60 - t]])
        if only_w_candidate(a, 0) and only_w_candidate(b, 0):
            return a, b
        attempt += 1


@pytest.mark.parametrize("t", [1, 3, 11])
def test_fp_length_only(S, torch, gpu_ctx, t):
    params = (32, FP_AVG, 60)
    objs = length_case(t)
    want = restate(S, objs, params)
    assert want == S.ChunkResult(2 * 92 - t, 4, 3, 32 + 60 + 60 - t, 2, 1)
    with gpu_ctx.chunker(*params) as h:
        for k, o in enumerate(objs):
            h.add(dev(torch, np.concatenate([o, np.full(16 + -len(o) % 16, 0xB1 + k, np.uint8)])), len(o))
        got = h.result()
    assert got == want


# ---- 12. pass C: one chunk far above 65 536 bytes -------------------------------------------------------

def test_fp_chunk_of_megabytes(S, torch, gpu_ctx):
    """Three objects of 4 MiB + 5 at avg = 2^24, max = 2^30: a wave walks 65 536 bitmap
    words in pass B and 4096 laps in pass C; one flipped bit at 3 MiB + 7 is seen."""
    params = (32, 1 << 24, 1 << 30)
    size = 4 * MiB + 5
    a = random_bytes(size, 90)
    b = a.copy()
    b[3 * MiB + 7] ^= 0x10
    objs = [a, b, a]
    want = restate(S, objs, params)
    assert want.chunks % 3 == 0 and want.unique_chunks == want.chunks // 3 + 1      # one chunk holds the flip
    assert want.bytes > MiB * want.chunks                                           # chunks of megabytes
    with gpu_ctx.chunker(*params) as h:
        for k, o in enumerate(objs):
            h.add(dev(torch, np.concatenate([o, np.full(11, 0x21 + k, np.uint8)])), size)
        got = h.result()
    assert got == want


# ---- 13. accumulation -----------------------------------------------------------------------------

def test_adds_accumulate(S, torch, gpu_ctx):
    size, n, stride = 30011, 4, 30016
    objs = [random_bytes(size, 50 + j) for j in range(n)]
    t = dev(torch, strided(objs, stride, 0))
    with gpu_ctx.chunker(*SMALL) as h:
        assert h.result() == S.ChunkResult()
        h.add_stream(t, size, n, stride)
        r1 = h.result()
        assert r1 == h.result() == restate(S, objs, SMALL)      # result() changes nothing
        h.add_stream(t, size, n, stride)                         # the same again: nothing new
        r2 = h.result()
        assert (r2.bytes, r2.chunks, r2.candidates, r2.forced_cuts) == \
            (2 * r1.bytes, 2 * r1.chunks, 2 * r1.candidates, 2 * r1.forced_cuts)
        assert (r2.unique_chunks, r2.unique_bytes) == (r1.unique_chunks, r1.unique_bytes)
        h.reset()
        assert h.result() == S.ChunkResult()
        h.add(t, size)
        assert h.result() == restate(S, objs[:1], SMALL)
        h.add_stream(0, 0, 5)                  # zero-length adds launch nothing, whatever the pointer
        h.add_stream(0, 4096, 0)
        assert h.result() == restate(S, objs[:1], SMALL)


def test_ring_overwritten_on_one_stream(S, torch, gpu_ctx):
    """Four payloads pass through one buffer on one stream, no sync between."""
    size = 200003
    parts = [random_bytes(size, 60 + k) for k in range(3)] + [random_bytes(size, 60)]
    srcs = [dev(torch, p) for p in parts]
    ring = torch.zeros(size + 13, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with gpu_ctx.chunker(*SMALL) as h:
        with torch.cuda.stream(st):
            for s in srcs:
                ring[:size].copy_(s, non_blocking=True)
                h.add(ring, size, stream=st)
        r = h.result()
    st.synchronize()
    assert r == restate(S, parts, SMALL)
    assert r.unique_bytes == 3 * size


def test_two_streams_two_threads(S, torch, gpu_ctx):
    parts = [random_bytes(300007, 70), random_bytes(MiB + 5, 1)]
    ts = [dev(torch, np.concatenate([p, np.zeros(16, np.uint8)])) for p in parts]
    torch.cuda.synchronize()               # the uploads ran on the default stream
    errs = []
    with gpu_ctx.chunker(*SMALL) as h:
        def work(k):
            try:
                st = torch.cuda.Stream()
                for _ in range(4):
                    h.add(ts[k], len(parts[k]), stream=st)
            except Exception as e:   # pragma: no cover
                errs.append(e)
        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs
        r = h.result()
    want = restate(S, parts, SMALL)
    assert (r.bytes, r.chunks, r.candidates, r.forced_cuts) == \
        (4 * want.bytes, 4 * want.chunks, 4 * want.candidates, 4 * want.forced_cuts)
    assert (r.unique_chunks, r.unique_bytes) == (want.unique_chunks, want.unique_bytes)


def test_array_growth(S, torch, gpu_ctx):
    """Many small chunks in adds of growing size: the handle's arrays double several times."""
    sizes = [1000, 50001, 100003, 200001, 400007, 700001]
    parts = [random_bytes(n, 80 + k) for k, n in enumerate(sizes)]
    with gpu_ctx.chunker(*SMALL) as h:
        for k, p in enumerate(parts):
            h.add(dev(torch, np.concatenate([p, np.zeros(16, np.uint8)])), len(p))
            if k == 2:
                assert h.result() == restate(S, parts[:3], SMALL)
        r = h.result()
    assert r == restate(S, parts, SMALL)
    assert sum(n // 32 + 2 for n in sizes) > 8 * 4096       # slots: at least three doublings from 4096


# ---- 14. host form ----------------------------------------------------------------------------------

def test_host_buffers(S):
    a = random_bytes(MiB + 5)
    want = restate(S, [a], SMALL)
    pad = np.zeros(a.size + 64, np.uint8)
    for off in (0, 1, 3, 17):                            # unaligned
        pad[off:off + a.size] = a
        assert S.measure_chunks_data(pad[off:off + a.size], *SMALL) == want, off
    assert S.measure_chunks_data(bytes(a), *SMALL) == want                         # read-only
    assert S.measure_chunks_data(memoryview(bytes(a)), *SMALL) == want
    ro = np.array(a)
    ro.setflags(write=False)
    assert S.measure_chunks_data(ro) == restate(S, [a], DEFAULTS)
    assert S.measure_chunks_data(b"", *SMALL) == S.ChunkResult()


def test_host_buffer_across_the_copy_edge(S):
    """More than one 64 MiB staging copy, a crafted window across the copy's edge."""
    w = window13()
    edge = 64 * MiB
    size = edge + 5003
    a = zeros_with(size, [edge - 40000, edge + 10, edge + 3000], w)
    want = restate(S, [a], DEFAULTS)
    assert want.candidates >= 3
    assert S.measure_chunks_data(a) == want
    b = np.empty(size + 1, np.uint8)
    b[1:] = a
    assert S.measure_chunks_data(b[1:]) == want          # unaligned: the edge falls elsewhere in the caller's memory


# ---- 15. refusals ------------------------------------------------------------------------------------

def test_refusals(S, torch, gpu_ctx):
    t = torch.zeros(3 * 4096 + 32, dtype=torch.uint8, device="cuda:0")
    for bad, msg in [((2048, 8000, 65536), "power of two"), ((2048, 32, 65536), "power of two"),
                     ((2048, 1 << 25, 1 << 26), "power of two"), ((31, 64, 256), "at least 32"),
                     ((300, 64, 256), "exceed max_bytes"), ((2048, 8192, (1 << 30) + 1), "2\\^30")]:
        with pytest.raises(ValueError, match=msg):
            gpu_ctx.chunker(*bad)
    with gpu_ctx.chunker() as h:
        with pytest.raises(ValueError, match="16-byte aligned"):
            h.add_stream(t[8:], 4096, 2, 4096)
        with pytest.raises(ValueError, match="16-byte aligned"):
            h.add_stream(t, 4096, 2, 4104)
        with pytest.raises(ValueError, match="overlap"):
            h.add_stream(t, 8192, 2, 4096)
        assert h.result() == S.ChunkResult()
    assert gpu_ctx.measure_chunks(t[:4096 + 16], 4096 + 16, 1 << 30, 1 << 24, 1 << 30).chunks == 1
