"""GPU: a mixed-size batch in one add of the three read-only analyses
(s3dg_measure_add_batch, s3dg_chunks_add_batch, s3dg_lz_add_batch and the
surfaces over them).

Every number is exact and has two judges.  The first is the restatement the
suites already use, on host bytes: a set of the blocks' bytes and
count_nonzero (tests/test_gpu_measure.py's `expect`), tests/lz_restatement.py,
and the chunk definition restated in tests/test_gpu_chunks.py.  The second is a
second handle fed object by object with the calls that existed before
(add_range of all blocks; for the chunker add_stream of one object), which is
the definition of a batch add.  Where a restatement would take minutes (tens
of megabytes of LZ parsing in Python) the second judge stands alone, or the
expected numbers are summed over the distinct objects of the batch.
"""
import ctypes
import functools
import threading

import numpy as np
import pytest

import lz_restatement as R
import test_gpu_chunks as TC
import test_gpu_measure as TM

pytestmark = pytest.mark.gpu

MiB = 1 << 20
GiB = 1 << 30
POISON = 0xA5
SMALL, DEFAULTS = TC.SMALL, TC.DEFAULTS
TILES = (2, 4, 8, 16, 32, 64, 0)   # s3dg_set_batch_tile: 0 = chosen per add


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---- the three handles behind one face ------------------------------------------------

class Kind:
    """A handle type with its parameters: how to open it, its restatement on
    host objects, and the add of one object with the calls that existed
    before the batch add."""

    def __init__(self, name, unit, open_, judge, one):
        self.name, self.unit, self.open, self.judge, self.one = name, unit, open_, judge, one

    def __repr__(self):
        return self.name


def measure_kind(bb, hist=False):
    return Kind(f"measure{bb}{'h' if hist else ''}", bb, lambda ctx: ctx.measurer(bb, hist),
                lambda S, objs: TM.expect(S, objs, bb, hist),
                lambda h, p, n, st: h.add_range(p, n, 0, -(-n // bb), stream=st))


def lz_kind(bb):
    return Kind(f"lz{bb}", bb, lambda ctx: ctx.lz_measurer(bb), lambda S, objs: S.LzResult(**R.measure(objs, bb)),
                lambda h, p, n, st: h.add_range(p, n, 0, -(-n // bb), stream=st))


def chunk_kind(params):
    return Kind("chunks%d_%d_%d" % params, params[2], lambda ctx: ctx.chunker(*params),
                lambda S, objs: TC.restate(S, objs, params),
                lambda h, p, n, st: h.add_stream(p, n, 1, stride=0, stream=st))


M4, M12, M68 = measure_kind(4096), measure_kind(12288), measure_kind(69632)
M4H = measure_kind(4096, hist=True)
L4, L12, L64 = lz_kind(4096), lz_kind(12288), lz_kind(65536)
CS, CD = chunk_kind(SMALL), chunk_kind(DEFAULTS)
ONE_EACH = [M4H, L4, CS]
ids = repr


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to("cuda:0")


def live(host, spans):
    """The non-empty spans' bytes of a host copy of the buffer."""
    return [host[o:o + n] for o, n in spans if n]


def batch(ctx, kind, t, spans, stream=None):
    with kind.open(ctx) as h:
        h.add_batch(t, spans, stream=stream)
        return h.result()


def each(ctx, kind, t, spans):
    """The second judge: one handle, one add per object."""
    with kind.open(ctx) as h:
        for o, n in spans:
            if n:
                kind.one(h, t.data_ptr() + o, n, None)
        return h.result()


def check(S, ctx, kind, t, host, spans, restated=True):
    got = batch(ctx, kind, t, spans)
    assert got == each(ctx, kind, t, spans), kind
    if restated:
        assert got == kind.judge(S, live(host, spans)), kind
    return got


def pack(sizes, first=16):
    """Spans at 16-byte offsets that are no multiple of 4096, at least 16
    bytes of gap behind each; and the buffer's length."""
    spans, off = [], first
    for n in sizes:
        if off % 4096 == 0:
            off += 16
        spans.append((off, n))
        off = (off + n + 15) // 16 * 16 + 16
    return spans, off


def scaled(r, k, unique):
    """Result r with every additive field k-fold and the unique_* fields kept."""
    import dataclasses
    d = {}
    for f in dataclasses.fields(r):
        v = getattr(r, f.name)
        if f.name in unique:
            d[f.name] = v
        elif isinstance(v, tuple):
            d[f.name] = tuple(k * x for x in v)
        else:
            d[f.name] = None if v is None else k * v
    return type(r)(**d)


UNIQUE = ("unique_blocks", "unique_chunks", "unique_bytes")


@functools.lru_cache(maxsize=None)
def random_bytes(size, seed=1):
    a = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    a.setflags(write=False)
    return a


# ---- 1. sizes ---------------------------------------------------------------------------

def size_list(unit):
    return [0, 1, 15, 16, 17, 4095, 4096, 4097, unit - 1, unit, unit + 1, 3 * unit + 5]


@pytest.fixture(scope="module")
def sized(S, torch, gpu_ctx):
    """For a unit (block_bytes or max_bytes): the size list three times, once
    per content (random bytes; controlled d2 c1.5 and DG1 payloads filled on
    the GPU with one seed each, so that blocks repeat across objects), packed
    at odd 16-byte offsets with poisoned gaps: (tensor, host copy, spans)."""
    cache = {}

    def get(unit):
        if unit not in cache:
            sizes = size_list(unit)
            spans, total = pack(sizes * 3)
            host = np.full(total, POISON, np.uint8)
            k = len(sizes)
            for j, (o, n) in enumerate(spans[:k]):
                host[o:o + n] = random_bytes(n, 100 + j)
            t = dev(torch, host)
            gpu_ctx.fill_batch(t, [(o, n, 7, 2, (3, 2)) for o, n in spans[k:2 * k]])
            for o, n in spans[2 * k:]:
                if n:
                    gpu_ctx.dgen_fill(t.data_ptr() + o, n, seed=5)
            torch.cuda.synchronize()
            host = t.cpu().numpy()
            inside = np.zeros(total, bool)
            for o, n in spans:
                inside[o:o + n] = True
            assert (host[~inside] == POISON).all()     # the fills left the gaps alone
            cache[unit] = (t, host, spans)
        return cache[unit]
    return get


@pytest.fixture(scope="module")
def wave_ctx(S, gpu_ctx):
    ctxs = {w: S.Context(0, base_seed=S.DEFAULT_BASE_SEED, waves_per_block=w) for w in (1, 2, 4)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("kind", [M4H, M12, M68], ids=ids)
def test_sizes_measure(S, torch, wave_ctx, sized, kind, waves):
    """Both pass-2 kernels (3 and 17 granules per block) at 1, 2 and 4 waves per
    granule; at 4096 with the histogram, which equals bincount over the spans' bytes."""
    t, host, spans = sized(kind.unit)
    r = check(S, wave_ctx[waves], kind, t, host, spans)
    assert r.blocks == sum(-(-n // kind.unit) for _, n in spans)
    if kind is M4H:
        assert r.hist == tuple(int(v) for v in np.bincount(np.concatenate(live(host, spans)), minlength=256))


@pytest.mark.parametrize("kind", [L4, L12, L64, CS, CD], ids=ids)
def test_sizes_lz_and_chunks(S, torch, gpu_ctx, sized, kind):
    t, host, spans = sized(kind.unit)
    check(S, gpu_ctx, kind, t, host, spans)


# ---- 2. tiles ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiled(S, torch):
    """For every tile size T: zeroed objects of T - 1, T and T + 1 granules,
    each followed by an empty span, with one marker byte in the first and the
    last live granule of the object's first tile, in the first granule of its
    second tile and in the object's last granule (its last byte)."""
    sizes, marks = [], []
    for T in (2, 4, 8, 16, 32, 64):
        for g in (T - 1, T, T + 1):
            n = g * 4096 - (5 if g != T else 0)
            sizes += [n, 0]
            marks.append([(0, 3), (min(T, g) - 1, 100), (g - 1, n - (g - 1) * 4096 - 1)] + ([(T, 7)] if g > T else []))
    spans, total = pack(sizes)
    host = np.full(total, POISON, np.uint8)
    v = 1
    for (o, n), m in zip(spans[::2], marks):
        host[o:o + n] = 0
        for g, b in m:
            host[o + g * 4096 + b] = v
            v = v % 255 + 1
    return dev(torch, host), host, spans


@pytest.fixture(scope="module")
def tiled_want(S, tiled):
    _, host, spans = tiled
    return {k.name: k.judge(S, live(host, spans)) for k in (M4H, M12, L4, CS)}


@pytest.mark.parametrize("tile", TILES)
def test_tiles(S, torch, gpu_ctx, tiled, tiled_want, tile):
    """Results are identical at every tile size, forced and chosen."""
    t, host, spans = tiled
    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    try:
        ctx.set_batch_tile(tile)
        for kind in (M4H, M12, L4, CS):
            assert batch(ctx, kind, t, spans) == tiled_want[kind.name], (kind, tile)
    finally:
        ctx.close()
    assert batch(gpu_ctx, CS, t, spans) == each(gpu_ctx, CS, t, spans)


# ---- 3. same content at different alignments ---------------------------------------------

@pytest.mark.parametrize("kind", [M4, M12, L4, CS, CD], ids=ids)
def test_same_content_at_two_alignments(S, torch, gpu_ctx, kind):
    """One object at offsets 16 and 2064 mod 4096: equal fingerprints, nothing new."""
    obj = random_bytes(3 * kind.unit + 5, 31)
    a, b = 4096 + 16, 64 * 4096 + 2064 + (3 * kind.unit + 4095) // 4096 * 4096
    host = np.full(b + obj.size + 16, POISON, np.uint8)
    host[a:a + obj.size] = obj
    host[b:b + obj.size] = obj
    t = dev(torch, host)
    assert a % 4096 == 16 and b % 4096 == 2064
    one = check(S, gpu_ctx, kind, t, host, [(a, obj.size)])
    two = check(S, gpu_ctx, kind, t, host, [(a, obj.size), (b, obj.size)])
    assert two == scaled(one, 2, UNIQUE)


# ---- 4. layout freedom -------------------------------------------------------------------

@pytest.mark.parametrize("kind", [M4H, M12, L4, CS], ids=ids)
def test_any_order_repeats_and_overlaps(S, torch, gpu_ctx, sized, kind):
    t, host, spans = sized(kind.unit)
    want = batch(gpu_ctx, kind, t, spans)
    assert batch(gpu_ctx, kind, t, spans[::-1]) == want
    shuffled = [spans[k] for k in np.random.default_rng(4).permutation(len(spans))]
    assert shuffled != spans and batch(gpu_ctx, kind, t, shuffled) == want
    # a uint64 array instead of tuples
    assert batch(gpu_ctx, kind, t, np.array(shuffled, np.uint64)) == want
    # every span twice: two objects each, nothing new among them
    twice = batch(gpu_ctx, kind, t, spans + spans)
    assert twice == scaled(want, 2, UNIQUE)
    assert twice == each(gpu_ctx, kind, t, spans + spans)
    # two overlapping spans are two objects
    o, n = max(spans, key=lambda s: s[1])
    d = min(n // 2, 4096 + 32) // 16 * 16
    over = [(o, n - 37), (o + d, n - d)]
    check(S, gpu_ctx, kind, t, host, over)


# ---- 5. gaps and neighbours ----------------------------------------------------------------

@pytest.mark.parametrize("last", [1, 17])
@pytest.mark.parametrize("kind", [M4H, L4, CS, CD], ids=ids)
def test_gaps_and_neighbours_are_not_read(S, torch, gpu_ctx, kind, last):
    """Every gap byte, the bytes before the first object and (there are none:
    the last object ends the buffer) after the last change; no field does."""
    sizes = [1, 4097, 17, 15, 3 * kind.unit + 5, 4095, 16, last]
    spans, _ = pack(sizes, first=64)
    total = spans[-1][0] + last
    inside = np.zeros(total, bool)
    host = np.full(total, POISON, np.uint8)
    for j, (o, n) in enumerate(spans):
        host[o:o + n] = random_bytes(n, 40 + j)
        inside[o:o + n] = True
    t = dev(torch, host)
    assert t.numel() == spans[-1][0] + spans[-1][1]
    want = check(S, gpu_ctx, kind, t, host, spans)
    for poison in (0x00, 0x3C):
        other = host.copy()
        other[~inside] = poison
        assert batch(gpu_ctx, kind, dev(torch, other), spans) == want


# ---- 6. many objects ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", [M4H, L4, CS], ids=ids)
def test_70000_spans(S, torch, gpu_ctx, kind):
    """Beyond a 65 535 grid limit; the judge is the same handle's add_stream."""
    n, size, stride = 70000, 100, 112
    rows = np.stack([random_bytes(size, 200 + k) for k in range(7)])
    host = np.full((n, stride), POISON, np.uint8)
    host[:, :size] = rows[np.arange(n) % 7]
    t = dev(torch, host.reshape(-1))
    spans = np.stack([np.arange(n, dtype=np.uint64) * stride, np.full(n, size, np.uint64)], axis=1)
    got = batch(gpu_ctx, kind, t, spans)
    with kind.open(gpu_ctx) as h:
        h.add_stream(t, size, n, stride)
        assert got == h.result()
    assert got.bytes == n * size
    if kind is M4H:
        assert (got.blocks, got.unique_blocks) == (n, 7)
    if kind is CS:
        small = TC.restate(S, list(rows), SMALL)
        assert got.unique_chunks == small.unique_chunks and got.chunks == small.chunks * n // 7


# ---- 7. 64-bit offsets -------------------------------------------------------------------

@pytest.mark.parametrize("kind", [M4H, L4, CS], ids=ids)
def test_spans_more_than_4_gib_apart(S, torch, gpu_ctx, kind):
    far = 4 * GiB + 4096 + 32
    a, b = random_bytes(70001, 7), random_bytes(69999, 8)
    t = torch.empty(far + b.size + 16, dtype=torch.uint8, device="cuda:0")   # the gap stays uninitialised
    t[16:16 + a.size] = torch.from_numpy(np.array(a)).to("cuda:0")
    t[far:far + b.size] = torch.from_numpy(np.array(b)).to("cuda:0")
    torch.cuda.synchronize()
    spans = [(far, b.size), (16, a.size)]
    got = batch(gpu_ctx, kind, t, spans)
    assert got == kind.judge(S, [b, a]) == each(gpu_ctx, kind, t, spans)


# ---- 8. sub-launch split -------------------------------------------------------------------

def test_more_than_2_22_granules(S, torch, gpu_ctx):
    """65 zeroed spans of 256 MiB + 12 293 bytes: 4 260 100 granules, two
    sub-launches of pass 1 (the cut falls inside span 63 at 64-granule tiles).
    Three marker bytes: in the last granule before the cut, in the first one
    behind it and in the batch's last granule.  Closed forms."""
    Z, n = 256 * MiB + 3 * 4096 + 5, 65
    spans, total = pack([Z] * n)
    per = -(-Z // 4096)                      # 65 540 granules, 1025 tiles of 64 per span
    cut_span, cut_tile = divmod((1 << 22) // 64, -(-per // 64))
    assert n * per > 1 << 22 and cut_span == 63 and 0 < cut_tile < 1024
    # a marker value whose 32 windows hold no candidate cut at 13 bits, so the chunks are forced cuts alone
    row = np.zeros((1, 96), np.uint8)
    row[0, 32] = 0xC3
    assert not TC.candidates(row, 13).any() and not TC.candidates(np.zeros((1, 96), np.uint8), 13).any()
    marks = [(cut_span, (cut_tile * 64 - 1) * 4096 + 100), (cut_span, cut_tile * 64 * 4096 + 200),
             (n - 1, Z - 3)]
    t = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    for j, b in marks:
        t[spans[j][0] + b] = 0xC3
    torch.cuda.synchronize()
    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    try:
        ctx.set_batch_tile(64)
        m = batch(ctx, M4, t, spans)
        c = batch(ctx, CD, t, spans)
    finally:
        ctx.close()
    # measure: the zero block, the ragged zero block, and three blocks with a marker at different places
    assert Z % 4096 == 5 and marks[2][1] // 4096 == per - 1
    assert m == S.MeasureResult(n * Z, n * Z - 3, n * per, 5, None)
    # chunks: 4096 forced chunks of 65 536 zeros and one ragged chunk per span; a marker makes its chunk distinct
    mx = DEFAULTS[2]
    assert c == S.ChunkResult(n * Z, n * (Z // mx + 1), 5, 3 * mx + 2 * (Z % mx), 0, n * (Z // mx))
    # lz at 65 536: sums over the distinct blocks
    lz = batch(gpu_ctx, L64, t, spans)
    nb = -(-Z // 65536)
    blocks = {(65536, ()): n * (nb - 1), (Z % 65536, ()): n}
    for j, p in marks:
        size = min(65536, Z - p // 65536 * 65536)
        blocks[(size, ())] -= 1
        blocks[(size, (p % 65536,))] = 1
    want = dict.fromkeys(R.FIELDS, 0)
    for (size, key), count in blocks.items():
        b = np.zeros(size, np.uint8)
        b[list(key)] = 0xC3
        one = R.measure([b], 65536)
        for f in R.FIELDS:
            want[f] += count * one[f]
    assert len(blocks) == 5 and lz == S.LzResult(**want)


# ---- 9. LZ: every wave takes blocks of several objects ---------------------------------------

@pytest.mark.parametrize("bb", [4096, 65536])
def test_lz_wave_reuse(S, torch, gpu_ctx, bb):
    """grid + 7 spans of 1, 2 and 3 blocks in turn with ragged ends, drawn
    from 7 contents: a wave's blocks w and w + grid belong to objects of
    different size."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * min(32, (160 * 1024) // (bb + 8192))
    n = grid + 7
    contents = [np.concatenate([random_bytes(bb + 100 * c, 300 + c), np.zeros(bb, np.uint8), random_bytes(bb, 310 + c)])
                for c in range(7)]
    kinds = {}
    for k in range(21):
        nb, c = k % 3 + 1, k % 7
        kinds[k] = contents[c][:(nb - 1) * bb + 1 + (997 * (c + 1)) % (bb - 1)]
    sizes = [kinds[k % 21].size for k in range(n)]
    assert len({a.size for a in kinds.values()}) == 21
    spans, total = pack(sizes)
    host = np.full(total, POISON, np.uint8)
    for k, (o, s) in enumerate(spans):
        host[o:o + s] = kinds[k % 21]
    owner = np.repeat(np.arange(n), [-(-s // bb) for s in sizes])
    assert owner.size > 2 * grid - 1
    w = np.arange(grid)
    w = w[w + grid < owner.size]
    size_of = np.array(sizes)
    assert (size_of[owner[w]] != size_of[owner[w + grid]]).all()
    got = batch(gpu_ctx, lz_kind(bb), dev(torch, host), spans)
    want = dict.fromkeys(R.FIELDS, 0)
    for k in range(21):
        one = R.measure([kinds[k]], bb)
        count = len(range(k, n, 21))
        for f in R.FIELDS:
            want[f] += count * one[f]
    assert got == S.LzResult(**want)


# ---- 10. chunker ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [CS, CD], ids=ids)
def test_chunker_short_forced_and_unequal_slots(S, torch, gpu_ctx, kind):
    """A span shorter than min_bytes, exactly max_bytes of zeros (one forced
    cut), and spans whose slot counts differ: slots past an object's chunk
    count yield no chunk."""
    mn, _, mx = (int(x) for x in kind.name[6:].split("_"))
    objs = [random_bytes(mn - 12, 1), np.zeros(mx, np.uint8), random_bytes(5 * mn + 3, 2), random_bytes(200 * mn, 3),
            np.zeros(3 * mx + 1, np.uint8), random_bytes(1, 4)]
    spans, total = pack([o.size for o in objs])
    host = np.full(total, POISON, np.uint8)
    for (o, n), a in zip(spans, objs):
        host[o:o + n] = a
    t = dev(torch, host)
    r = check(S, gpu_ctx, kind, t, host, spans)
    assert batch(gpu_ctx, kind, t, [spans[0]]).chunks == 1
    z = batch(gpu_ctx, kind, t, [spans[1]])
    assert (z.chunks, z.forced_cuts, z.unique_chunks, z.candidates) == (1, 1, 1, 0)
    assert r.chunks < sum(-(-n // mn) + 1 for _, n in spans)       # fewer chunks than slots


# ---- 11. accumulation ------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ONE_EACH, ids=ids)
def test_batch_stream_and_range_adds_accumulate(S, torch, gpu_ctx, sized, kind):
    t, host, spans = sized(kind.unit)
    objs = live(host, spans)
    size, n, stride = 30011, 4, 30016
    sobjs = [random_bytes(size, 50 + j) for j in range(n)]
    st = dev(torch, TC.strided(sobjs, stride, 0))
    lone = random_bytes(3 * kind.unit + 77, 9)
    lt = dev(torch, np.concatenate([lone, np.zeros(16, np.uint8)]))
    with kind.open(gpu_ctx) as h:
        assert h.result().bytes == 0
        h.add_batch(t, spans)
        r1 = h.result()
        assert r1 == h.result() == kind.judge(S, objs)                   # result() changes nothing
        h.add_stream(st, size, n, stride)
        assert h.result() == kind.judge(S, objs + sobjs)
        kind.one(h, lt.data_ptr(), lone.size, None)
        assert h.result() == kind.judge(S, objs + sobjs + [lone])
        h.add_batch(t, [])                                                 # nothing, whatever else
        h.add_batch(0, [(8, 0), (0, 0)])
        h.add_batch(t, spans)                                              # the same batch again: nothing new
        r2 = h.result()
        assert r2 == kind.judge(S, objs + sobjs + [lone] + objs)
        h.reset()
        r0 = h.result()
        assert r0.bytes == 0 and r0 == scaled(r1, 0, ())
        h.add_batch(t, spans)
        h.add_batch(t, spans)
        assert h.result() == scaled(r1, 2, UNIQUE)


@pytest.mark.parametrize("kind", ONE_EACH, ids=ids)
def test_ring_overwritten_between_batch_adds(S, torch, gpu_ctx, kind):
    """Three payloads pass through one buffer on one stream, no sync between."""
    spans, total = pack([50001, 0, 4097, 17, 3 * kind.unit + 5])
    parts = [random_bytes(total, 60 + k) for k in range(3)]
    srcs = [dev(torch, p) for p in parts]
    ring = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with kind.open(gpu_ctx) as h:
        with torch.cuda.stream(st):
            for s in srcs:
                ring.copy_(s, non_blocking=True)
                h.add_batch(ring, spans, stream=st)
        r = h.result()
    st.synchronize()
    assert r == kind.judge(S, [o for p in parts for o in live(p, spans)])


@pytest.mark.parametrize("kind", ONE_EACH, ids=ids)
def test_two_streams_two_threads(S, torch, gpu_ctx, sized, kind):
    t, host, spans = sized(kind.unit)
    halves = [spans[::2], spans[1::2]]
    torch.cuda.synchronize()
    errs = []
    with kind.open(gpu_ctx) as h:
        def work(k):
            try:
                st = torch.cuda.Stream()
                for _ in range(4):
                    h.add_batch(t, halves[k], stream=st)
            except Exception as e:   # pragma: no cover
                errs.append(e)
        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs
        r = h.result()
    assert r == scaled(batch(gpu_ctx, kind, t, spans), 4, UNIQUE)


@pytest.mark.parametrize("kind", ONE_EACH, ids=ids)
def test_growth_over_four_doublings(S, torch, gpu_ctx, kind):
    """Adds of 5000, 10 000, 20 000 and 40 000 one-block objects: the handle's
    arrays double at least four times from 4096 slots.  The judge is a second
    handle with add_stream over the same bytes."""
    counts, size, stride = [5000, 10000, 20000, 40000], 40, 48
    n = sum(counts)
    host = np.random.default_rng(5).integers(0, 256, (n, stride), dtype=np.uint8)
    host[::3, :size] = host[0, :size]                     # every third object is the first again
    t = dev(torch, host.reshape(-1))
    assert n > 16 * 4096
    with kind.open(gpu_ctx) as h, kind.open(gpu_ctx) as j:
        lo = 0
        for k, c in enumerate(counts):
            spans = np.stack([np.arange(lo, lo + c, dtype=np.uint64) * stride, np.full(c, size, np.uint64)], axis=1)
            h.add_batch(t, spans)
            j.add_stream(t.data_ptr() + lo * stride, size, c, stride)
            lo += c
            if k == 1:
                assert h.result() == j.result()
        got = h.result()
        assert got == j.result() and got.bytes == n * size
    if kind is M4H:
        assert got.blocks == n and got.unique_blocks == n - len(range(0, n, 3)) + 1


@pytest.mark.parametrize("sym, kind", [("measure", M4H), ("lz", L4), ("chunks", CS)], ids=["measure", "lz", "chunks"])
def test_span_array_is_consumed_before_return(S, torch, gpu_ctx, sized, sym, kind):
    from s3dlio_amd import _lib
    t, host, spans = sized(kind.unit)
    arr = (_lib.Span * len(spans))(*[_lib.Span(o, n) for o, n in spans])
    st = torch.cuda.Stream()
    with kind.open(gpu_ctx) as h:
        for _ in range(4):
            for k, (o, n) in enumerate(spans):
                arr[k] = _lib.Span(o, n)
            _lib.call(f"s3dg_{sym}_add_batch", h._h, t.data_ptr(), arr, len(spans), st.cuda_stream)
            ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))           # garbage right after the call returns
        r = h.result()
    assert r == scaled(batch(gpu_ctx, kind, t, spans), 4, UNIQUE)


# ---- 12. refusals ---------------------------------------------------------------------------

@pytest.mark.parametrize("sym, kind", [("measure", M4H), ("lz", L4), ("chunks", CS)], ids=["measure", "lz", "chunks"])
def test_refusals(S, torch, gpu_ctx, sized, sym, kind):
    """Every refusal with its message, on a handle that already holds data:
    its result afterwards is its result before, and the buffer is untouched."""
    from s3dlio_amd import _lib
    t, host, spans = sized(kind.unit)
    p = t.data_ptr()

    def raw(ptr, rows, n=None, null=False):
        arr = (_lib.Span * max(1, len(rows)))(*[_lib.Span(o, s) for o, s in rows])
        _lib.call(f"s3dg_{sym}_add_batch", h._h, ptr, None if null else arr, len(rows) if n is None else n, None)

    with kind.open(gpu_ctx) as h:
        h.add_batch(t, spans)
        before = h.result()
        cases = [
            (lambda: raw(p, [], n=3, null=True), "null span array"),
            (lambda: raw(0, [(16, 5)]), "src_base must be a 16-byte aligned device pointer"),
            (lambda: raw(p + 8, [(16, 5)]), "src_base must be a 16-byte aligned device pointer"),
            (lambda: raw(p, [(16, 5), (8, 0), (32, 9), (24, 5), (40, 5)]), "span 3: off must be a multiple of 16"),
            (lambda: raw(p, [(8, 0), (16, 5), (32, (1 << 43) + 1), (24, 5)]), "span 2: object larger than 2^31 blocks"),
            (lambda: raw(p, [(16, 5), (2**64 - 16, 32)]), "span 1: off + size overflows"),
            (lambda: raw(p, [(0, 1 << 43)] * 513), "span 0: more than 2^31 - 1 chunk slots in one add"
             if sym == "chunks" else "span 512: more than 2^40 granules in one add"),
        ]
        if sym == "chunks":
            cases.append((lambda: raw(p, [(0, 32 * (2**31 - 3)), (0, 1)]),
                          "span 1: more than 2^31 - 1 chunk slots in one add"))
        for call, text in cases:
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == text
            assert h.result() == before
        # Python checks off + size against the tensor before any launch
        for rows in ([(16, t.numel())], [(0, 5), (t.numel() - 16, 17)], [(2**64 - 16, 32)]):
            with pytest.raises(ValueError, match="the call reads"):
                h.add_batch(t, rows)
        h.add_batch(t, [(t.numel() - 16, 16), (t.numel() + 4096, 0)])     # the last bytes; an empty span anywhere
        assert h.result().bytes == before.bytes + 16
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == host).all()


# ---- 13. one-shot forms ----------------------------------------------------------------------

def test_one_shot_forms(S, torch, gpu_ctx):
    """Config 4's size distribution scaled down: 64 log-uniform objects of 1
    byte to 3 MiB, d2 c1.5, fill_batch's tuples handed on unchanged."""
    rng = np.random.default_rng(44)
    sizes = [int(x) for x in np.exp(rng.uniform(0, np.log(3 * MiB), 64))]
    sizes[0], sizes[-1] = 1, 3 * MiB
    spans, total = pack(sizes)
    objects = [(o, n, 1000 + k, 2, (3, 2)) for k, (o, n) in enumerate(spans)]
    t = torch.full((total,), POISON, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.fill_batch(t, objects)
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    m = gpu_ctx.measure_batch(t, objects, hist=True)
    assert m == TM.expect(S, live(host, spans), 4096, True) == each(gpu_ctx, M4H, t, spans)
    assert gpu_ctx.measure_batch(t, objects, block_bytes=69632) == each(gpu_ctx, M68, t, spans)
    assert gpu_ctx.measure_chunks_batch(t, objects) == each(gpu_ctx, CD, t, spans)
    assert gpu_ctx.measure_chunks_batch(t, objects, *SMALL) == each(gpu_ctx, CS, t, spans)
    assert gpu_ctx.measure_lz_batch(t, objects) == each(gpu_ctx, L64, t, spans)
    assert gpu_ctx.measure_lz_batch(t, objects, block_bytes=4096) == each(gpu_ctx, L4, t, spans)
    small = [k for k, n in enumerate(sizes) if n <= 65536]
    sub = [spans[k] for k in small]
    assert gpu_ctx.measure_lz_batch(t, [objects[k] for k in small]) == S.LzResult(**R.measure(live(host, sub), 65536))
