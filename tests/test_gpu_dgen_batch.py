"""GPU: a mixed-size batch of DG1 objects in one call: s3dg_dgen_fill_batch /
Context.dgen_fill_batch (k_keystream_batch) and s3dg_verify_dgen_batch /
Context.verify_dgen_batch (k_verify_keystream_batch).

Expected bytes come only from the C oracle (oracle_c.dgen_fill), never from the
library's fill.  Every buffer is poisoned first and compared whole, so every
byte outside the objects must still hold the poison.  The expected verify
results come from numpy (`expect`): differing bytes, differing 4 KiB granules
within each object and the lowest offset.  Every comparison is exact.

Lane paths: the min_lane_draws knob of set_keystream_shape(1, ...) sets the
lanes of a full 1 MiB chunk: 131072 draws = 1 lane (no jump), 4096 = 32 lanes
(per-lane jump, two chunks per wave), 512 = 256 lanes (a chunk over four
waves).  2048 is the default, so the library reads it as "not set" and spreads
these small lists further: a chunk still takes at least 64 lanes, the scalar
jump.  The ragged classes get proportionally fewer lanes, down to one.

The implementation splits a call nowhere: one record table, one launch per
size class, and a class beyond the grid's reach is refused by the plan
(tests/test_dgen_batch_cpu.py), so there is no launch boundary to straddle.
"""
import ctypes
import functools
import random
import threading

import numpy as np
import pytest

from dgen_batch_cases import layout   # moved there unchanged: the CPU suite builds lists with it too

pytestmark = pytest.mark.gpu

MIB = 1 << 20
POISON = 0xA7
KNOBS = (131072, 4096, 2048, 512)
EDGE_SIZES = [0, 1, 4, 5, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097, 65536 + 3, MIB - 1, MIB, MIB + 1, MIB + 5,
              2 * MIB + 4097, 3 * MIB + 3]
COMPRESS = [1, 2, 3, (3, 2)]
DEDUPS = [1, 2, 3]


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
    """One context per min_lane_draws value."""
    out = {}
    for k in KNOBS:
        c = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
        c.set_keystream_shape(1, min_lane_draws=k)
        out[k] = c
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def dgen(S, oracle):
    """Oracle bytes, computed once per argument set and never modified."""
    @functools.lru_cache(maxsize=None)
    def f(size, dedup, compress, seed):
        fn, fd = S.compress_ratio(compress)
        a = oracle.dgen_fill(size, dedup, fn, fd, seed)
        a.setflags(write=False)
        return a
    return f


def edge_objects(params, seed0=0x5EED, extra=()):
    rng = random.Random(seed0)
    mid = EDGE_SIZES[1:] + list(extra)
    rng.shuffle(mid)
    sizes = [0] + mid[:9] + [0] + mid[9:] + [0]          # empty objects first, in the middle and last
    return layout(sizes, params, seed0, rng)


def mixed_objects(extra=()):
    """Parameters mixed per object (dedup bites from 3 blocks up)."""
    combos = [(d, c) for d in DEDUPS for c in COMPRESS]
    return edge_objects(lambda k: combos[(5 * k + 1) % len(combos)], seed0=0xD1CE, extra=extra)


def want_of(dgen, objs, total):
    want = np.full(total, POISON, np.uint8)
    for off, size, seed, dd, comp in objs:
        if size:
            want[off:off + size] = dgen(size, dd, comp, seed)
    return want


def poisoned(torch, total):
    return torch.full((total,), POISON, dtype=torch.uint8, device="cuda:0")


def clean(S, n, per_object=True):
    return S.BatchVerifyResult(S.VerifyResult(), n, () if per_object else None)


def filled(torch, S, dgen, ctx, objs, total, want=None):
    """Fills a poisoned buffer, compares it whole with the oracle (the poison
    outside the objects included) and verifies it clean.  Returns (tensor, want)."""
    if want is None:
        want = want_of(dgen, objs, total)
    t = poisoned(torch, total)
    ctx.dgen_fill_batch(t, objs)
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")
    assert ctx.verify_dgen_batch(t, objs) == clean(S, len(objs))
    return t, want


def expect(S, dgen, objs, got, per_object=True):
    """What verifying `got` (numpy) against the descriptors must report."""
    nbytes = nblocks = 0
    first = None
    mism = []
    for k, (off, size, seed, dd, comp) in enumerate(objs):
        if not size:
            continue
        bad = np.flatnonzero(got[off:off + size] != dgen(size, dd, comp, seed))
        if bad.size:
            g = int(np.unique(bad // 4096).size)
            mism.append((k, S.VerifyResult(int(bad.size), g, int(bad[0]))))
            nbytes += int(bad.size)
            nblocks += g
            first = off + int(bad[0]) if first is None else min(first, off + int(bad[0]))
    return S.BatchVerifyResult(S.VerifyResult(nbytes, nblocks, first), len(objs), tuple(mism) if per_object else None)


# ---- 1. fill: edges -----------------------------------------------------------------

@pytest.mark.parametrize("dedup", DEDUPS)
@pytest.mark.parametrize("compress", COMPRESS, ids=lambda c: f"c{c}")
def test_edges(S, torch, gpu_ctx, dgen, compress, dedup):
    """Every edge size in one shuffled list, at each ratio and dedup: the bytes
    are the oracle's, nothing else is written, and the verify finds it clean."""
    objs, total = edge_objects(lambda k: (dedup, compress))
    assert all(o[0] % 16 == 0 and o[0] % 4096 for o in objs) and len({o[2] for o in objs}) == len(objs)
    filled(torch, S, dgen, gpu_ctx, objs, total)


def test_mixed_parameters(S, torch, gpu_ctx, dgen):
    objs, total = mixed_objects()
    assert len({(o[3], o[4]) for o in objs}) >= 8
    filled(torch, S, dgen, gpu_ctx, objs, total)


# ---- 2. fill: lane paths, stage widths, workgroup shapes, store policies ---------------

@pytest.mark.parametrize("knob", KNOBS)
def test_lane_paths(S, torch, ctxs, dgen, knob):
    """The mixed list on each lane path, at draws 16/32/64 x waves 1/2/4 and at
    each store policy: the bytes are identical throughout."""
    ctx = ctxs[knob]
    objs, total = mixed_objects()
    want = want_of(dgen, objs, total)
    want_dev = torch.from_numpy(want).to("cuda:0")
    try:
        filled(torch, S, dgen, ctx, objs, total, want)
        shapes = [(d, w, -1) for d in (16, 32, 64) for w in (1, 2, 4)] + [(0, 0, sp) for sp in (0, 1, 2, 3)]
        for draws, waves, store in shapes:
            ctx.set_keystream_shape(1, draws=draws, waves=waves, min_lane_draws=knob, store_policy=store)
            t = poisoned(torch, total)
            ctx.dgen_fill_batch(t, objs)
            assert torch.equal(t, want_dev), (knob, draws, waves, store)
            assert ctx.verify_dgen_batch(t, objs, per_object=False) == clean(S, len(objs), False)
    finally:
        ctx.set_keystream_shape(1, min_lane_draws=knob)


# ---- 3. several objects in one wave ------------------------------------------------------

def small_objects():
    rng = random.Random(600)
    sizes = [2064 if k % 2 == 0 else 4096 + 16 for k in range(600)]
    return layout(sizes, lambda k: (1, 1 if k % 3 else 2), 0x600D, rng)


def test_many_small_objects(S, torch, gpu_ctx, dgen):
    """300 objects of 2064 bytes and 300 of 4096 + 16, interleaved: one lane
    each at the smallest class, so a wave serves 64 objects.  Bytes match the
    oracle, and each object equals dgen_fill on the device."""
    objs, total = small_objects()
    assert len({o[2] for o in objs}) == 600
    t, _ = filled(torch, S, dgen, gpu_ctx, objs, total)
    u = poisoned(torch, total)
    for off, size, seed, dd, comp in objs:
        gpu_ctx.dgen_fill(u[off:], size, dedup=dd, compress=comp, seed=seed)
    assert torch.equal(t, u)


# ---- 4. equivalence ------------------------------------------------------------------------

def test_equals_stream_and_is_order_free(S, torch, gpu_ctx, dgen):
    size, n, seed = 2 * MIB + 17, 8, 0xABCDEF
    stride = (size + 15) // 16 * 16 + 48
    total = n * stride
    for dd, comp in ((1, 1), (2, 2)):
        objs = [(j * stride, size, S.object_entropy(seed, j), dd, comp) for j in range(n)]
        a, b = poisoned(torch, total), poisoned(torch, total)
        gpu_ctx.dgen_fill_stream(a, size, n, stride=stride, dedup=dd, compress=comp, seed_base=seed)
        gpu_ctx.dgen_fill_batch(b, objs)
        assert torch.equal(a, b)
        assert gpu_ctx.verify_dgen_batch(a, objs) == clean(S, n)
        assert gpu_ctx.verify_dgen_stream(b, size, n, stride=stride, dedup=dd, compress=comp, seed_base=seed).ok
    objs, total = mixed_objects()
    t, want = filled(torch, S, dgen, gpu_ctx, objs, total)
    gpu_ctx.dgen_fill_batch(t, objs[::-1])                      # again, in reverse order
    assert np.array_equal(t.cpu().numpy(), want)
    assert gpu_ctx.verify_dgen_batch(t, objs[::-1]) == clean(S, len(objs))


# ---- 5. verify: clean ------------------------------------------------------------------------

def test_gap_bytes_are_not_read(S, torch, gpu_ctx, dgen):
    """Overwriting every byte outside the objects keeps the verify clean."""
    objs, total = mixed_objects()
    t, want = filled(torch, S, dgen, gpu_ctx, objs, total)
    inside = np.zeros(total, bool)
    for off, size, *_ in objs:
        inside[off:off + size] = True
    a = want.copy()
    a[~inside] ^= 0xFF
    t = torch.from_numpy(a).to("cuda:0")
    assert gpu_ctx.verify_dgen_batch(t, objs) == clean(S, len(objs))
    assert np.array_equal(t.cpu().numpy(), a)                   # and nothing is written


# ---- 6. verify: dirty ---------------------------------------------------------------------------

def flip_sites(objs):
    """(offset in the buffer, what) of the bit flips: an object's first and last
    byte, both sides of a zero prefix's end and of a 1 MiB block boundary."""
    big = next(o for o in objs if o[1] == 3 * MIB + 3)
    pre = next(o for o in objs if o[1] >= MIB and o[4] != 1)    # an object with a zero prefix
    fn, fd = (1, 2) if pre[4] == 2 else (2, 3) if pre[4] == 3 else (1, 3)
    z = MIB * fn // fd                                          # the first block's prefix
    small = next(o for o in objs if o[1] == 4096 + 16)
    return [(big[0], "first byte"), (big[0] + big[1] - 1, "last byte"),
            (pre[0] + z - 1, "prefix end"), (pre[0] + z, "after the prefix"),
            (big[0] + MIB - 1, "block end"), (big[0] + MIB, "block start"),
            (small[0] + 4096 + 15, "last byte of 4096 + 16")]


@pytest.mark.parametrize("knob", KNOBS)
def test_flips(S, torch, ctxs, dgen, knob):
    """One flipped bit per site, in separate runs and then all at once: the
    object, its bytes, granules and first offset are numpy's, per object and in
    the totals, and every other object is clean."""
    ctx = ctxs[knob]
    objs, total = mixed_objects(extra=[4096 + 16])
    want = want_of(dgen, objs, total)
    sites = flip_sites(objs)
    assert len({p for p, _ in sites}) == len(sites)
    t = torch.from_numpy(want).to("cuda:0")
    for p, what in sites:
        t[p] ^= 0x10
        got = want.copy()
        got[p] ^= 0x10
        r = ctx.verify_dgen_batch(t, objs)
        assert r == expect(S, dgen, objs, got), (knob, what)
        assert r.total.mismatched_bytes == 1 and r.mismatched_objects == 1, what
        t[p] ^= 0x10
    got = want.copy()
    for p, _ in sites:
        t[p] ^= 0x10
        got[p] ^= 0x10
    e = expect(S, dgen, objs, got)
    assert e.total.mismatched_bytes == len(sites)
    assert ctx.verify_dgen_batch(t, objs) == e
    assert ctx.verify_dgen_batch(t, objs, per_object=False) == expect(S, dgen, objs, got, False)
    assert np.array_equal(t.cpu().numpy(), got)                 # nothing is written


def test_last_byte_of_a_4112_byte_object(S, torch, gpu_ctx, dgen):
    """Every 7th of the 600 small objects corrupted (the 4096 + 16 ones in their
    last byte, the second granule): exactly those objects are named."""
    objs, total = small_objects()
    want = want_of(dgen, objs, total)
    got = want.copy()
    for k in range(0, 600, 7):
        off, size = objs[k][0], objs[k][1]
        got[off + size - 1] ^= 0x80
        if k % 2 == 0:
            got[off + 5] ^= 0x01
    t = torch.from_numpy(got).to("cuda:0")
    e = expect(S, dgen, objs, got)
    assert [k for k, _ in e.mismatches] == list(range(0, 600, 7))
    assert any(v.mismatched_blocks == 1 and v.first_offset == 4111 for _, v in e.mismatches)
    assert gpu_ctx.verify_dgen_batch(t, objs) == e


# ---- 7. verify: semantics --------------------------------------------------------------------------

def test_semantics(S, torch, gpu_ctx, dgen):
    objs, total = mixed_objects()
    want = want_of(dgen, objs, total)
    k = next(i for i, o in enumerate(objs) if o[1] == 2 * MIB + 4097)
    got = want.copy()
    got[objs[k][0] + MIB + 77] ^= 0x04
    got[objs[k][0] + 3] ^= 0x40
    t = torch.from_numpy(got).to("cuda:0")
    # a descriptor given twice counts twice and appears at both indices
    twice = objs + [objs[k]]
    r = gpu_ctx.verify_dgen_batch(t, twice)
    assert r == expect(S, dgen, twice, got)
    assert r.total.mismatched_bytes == 4 and [i for i, _ in r.mismatches] == [k, len(objs)]
    # reverse order: the same totals
    assert gpu_ctx.verify_dgen_batch(t, twice[::-1]).total == r.total
    assert gpu_ctx.verify_dgen_batch(t, twice, per_object=False) == expect(S, dgen, twice, got, False)
    # a wrong seed, dedup or compress makes only that object dirty, with numpy's counts
    t = torch.from_numpy(want).to("cuda:0")
    j = next(i for i, o in enumerate(objs) if o[1] == 3 * MIB + 3)
    off, size, seed, dd, comp = objs[j]
    for other in ((off, size, seed ^ 1, dd, comp), (off, size, seed, 1 if dd != 1 else 3, comp),
                  (off, size, seed, dd, 2 if comp != 2 else 3)):
        alt = objs[:j] + [other] + objs[j + 1:]
        r = gpu_ctx.verify_dgen_batch(t, alt)
        assert r == expect(S, dgen, alt, want), other
        assert [i for i, _ in r.mismatches] == [j] and r.total.mismatched_bytes > 1000


def test_two_threads_two_streams(S, torch, gpu_ctx, dgen):
    """Disjoint lists on two streams from two threads: both come out right."""
    objs, total = mixed_objects()
    half = [objs[0::2], objs[1::2]]
    want = want_of(dgen, objs, total)
    t = poisoned(torch, total)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    res, errs = [None, None], []

    def work(i):
        try:
            for _ in range(4):
                gpu_ctx.dgen_fill_batch(t, half[i], stream=streams[i])
                res[i] = gpu_ctx.verify_dgen_batch(t, half[i], stream=streams[i])
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    torch.cuda.synchronize()
    for s in streams:
        gpu_ctx.release_stream(s)
    assert not errs, errs
    assert res[0] == clean(S, len(half[0])) and res[1] == clean(S, len(half[1]))
    assert np.array_equal(t.cpu().numpy(), want)


# ---- 8. with the measure ------------------------------------------------------------------------------

def test_measure_batch_over_a_dgen_batch(S, torch, gpu_ctx, dgen):
    """measure_batch at 1 MiB blocks over a filled d3 c2 list: the distinct and
    zero counts of a Python set over the oracle bytes."""
    objs, total = edge_objects(lambda k: (3, 2), seed0=0xBEEF)
    t, want = filled(torch, S, dgen, gpu_ctx, objs, total)
    blocks, zeros, nblk, nbytes = set(), 0, 0, 0
    for off, size, *_ in objs:
        a = want[off:off + size]
        zeros += int(np.count_nonzero(a == 0))
        nbytes += size
        for b in range(0, size, MIB):
            blocks.add(a[b:b + MIB].tobytes())
            nblk += 1
    m = gpu_ctx.measure_batch(t, [(o[0], o[1]) for o in objs], block_bytes=MIB)
    assert (m.bytes, m.blocks, m.unique_blocks, m.zero_bytes) == (nbytes, nblk, len(blocks), zeros)
    assert len(blocks) < nblk                                   # dedup 3 bit on the 3-block object


# ---- 9. refusals -----------------------------------------------------------------------------------------

def test_refusals(S, torch, gpu_ctx, dgen):
    """Each refusal with its message and index; a refused fill leaves the
    poisoned buffer as it was, a refused verify leaves `out` and `per_obj`."""
    from s3dlio_amd import _lib
    D = _lib.ObjDesc
    total = 4 * 8192
    t = poisoned(torch, total)
    good = [D(16 + 8192 * k, 5000, k + 1, 1, 0, 1) for k in range(4)]
    p = t.data_ptr()

    def refused(msg, base, descs, n, out=True):
        arr = (D * max(1, len(descs)))(*descs) if descs is not None else None
        with pytest.raises(ValueError) as ei:
            _lib.call("s3dg_dgen_fill_batch", gpu_ctx._h, base, arr, n, 0)
        if msg != "null output":
            assert str(ei.value).endswith(msg.replace("src_base", "dst_base")), (msg, str(ei.value))
        tot, rec = _lib.VerifyRec(), (_lib.VerifyRec * 8)()
        ctypes.memset(ctypes.byref(tot), 0x5A, ctypes.sizeof(tot))
        ctypes.memset(rec, 0x5A, ctypes.sizeof(rec))
        with pytest.raises(ValueError) as ei:
            _lib.call("s3dg_verify_dgen_batch", gpu_ctx._h, base, arr, n, 0, ctypes.byref(tot) if out else None, rec)
        assert str(ei.value).endswith(msg), (msg, str(ei.value))
        assert bytes(tot) == b"\x5a" * 24 and bytes(rec) == b"\x5a" * 192      # written only on success

    refused("null descriptor array", p, None, 4)
    refused("src_base must be 16-byte aligned", None, good, 4)
    refused("src_base must be 16-byte aligned", p + 8, good, 4)
    bad = {"dst_off must be a multiple of 16": D(8, 100, 1, 1, 0, 1), "need f_num < f_den": D(0, 100, 1, 1, 3, 3),
           "object larger than 2^32 blocks": D(0, ((1 << 32) + 1) * MIB, 1, 1, 0, 1)}
    for msg, b in bad.items():
        for at in range(4):                                   # the first descriptor, the last, in between
            refused(f"object {at}: {msg}", p, good[:at] + [b] + good[at + 1:], 4)
    refused("object 3: need f_num < f_den", p, good[:3] + [D(0, 100, 1, 1, 0, 0)], 4)            # f_den == 0
    two = list(bad.values())
    refused("object 1: dst_off must be a multiple of 16", p, good[:1] + [two[0], two[1]] + good[3:], 4)
    refused("object 1: need f_num < f_den", p, good[:1] + [two[1], two[0]] + good[3:], 4)
    many = good * 5000 + [two[1]]                             # far behind valid work: still nothing has run
    refused("object 20000: need f_num < f_den", p, many, len(many))
    # the verify alone: a null output, whatever else
    tot = _lib.VerifyRec()
    arr = (D * 4)(*good)
    for n in (4, 0):
        with pytest.raises(ValueError, match="null output"):
            _lib.call("s3dg_verify_dgen_batch", gpu_ctx._h, p, arr, n, 0, None, None)
    torch.cuda.synchronize()
    assert bool((t == POISON).all())                          # no refused fill wrote anything
    # n == 0 and only empty objects launch nothing and succeed
    _lib.call("s3dg_dgen_fill_batch", gpu_ctx._h, None, None, 0, 0)
    _lib.call("s3dg_verify_dgen_batch", gpu_ctx._h, None, None, 0, 0, ctypes.byref(tot), None)
    assert (tot.mismatched_bytes, tot.mismatched_blocks, tot.first_offset) == (0, 0, 2**64 - 1)
    empties = [(8, 0, 1, 1, 1)] * 3                           # an empty object may say anything
    gpu_ctx.dgen_fill_batch(t, empties)
    assert gpu_ctx.verify_dgen_batch(t, empties) == clean(S, 3)
    torch.cuda.synchronize()
    assert bool((t == POISON).all())
    # the Python methods: bounds against the tensor before any call
    with pytest.raises(ValueError, match="writes"):
        gpu_ctx.dgen_fill_batch(t, [(16, 100, 1, 1, 1), (total - 100, 101, 1, 1, 1)])
    with pytest.raises(ValueError, match="reads"):
        gpu_ctx.verify_dgen_batch(t, [(total - 100, 101, 1, 1, 1)])
    with pytest.raises(ValueError, match="object 1: dst_off must be a multiple of 16"):
        gpu_ctx.dgen_fill_batch(t, [(16, 100, 1, 1, 1), (8, 100, 2, 1, 1)])
    assert bool((t == POISON).all())
    objs = [(16, 100, 1, 1, 1), (8192 + 16, 5000, 2, 1, 2)]   # and the context still works
    filled(torch, S, dgen, gpu_ctx, objs, total)
