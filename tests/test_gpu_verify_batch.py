"""GPU: s3dg_verify_controlled_batch / Context.verify_batch (k_verify_batch),
the read-side twin of fill_batch with a result per object.

Expected bytes are the C oracle's, uploaded into a buffer of 0xAB guards; the
judge is numpy (`judge`): per object bad = got != expected, bytes bad.sum(),
blocks the distinct idx // 4096, first idx.min(); totals are the sums and
min(off + first).  Every number is exact.  Guard and gap bytes are ordinary
allocated memory: "never reads past an object's end" is shown by changing them
and getting the same result.  A corrupted byte is `^= 0xFF`, so it always
differs."""
import ctypes
import functools
import math
import random
import threading

import numpy as np
import pytest

from oracle import oracle_py as P

pytestmark = pytest.mark.gpu

SEED_BASE = 0x5EED000000000001
GUARD = 0xAB
BLK = 4096
KiB, MiB = 1 << 10, 1 << 20
TILES = (0, 2, 4, 8, 16, 32, 64)          # 0: chosen per sub-batch (8..64); the rest forced
MAX_GRID = 1 << 22                        # slots per sub-launch

# the contract's refusal texts (include/s3dlio_gpu.h)
REFUSALS = ["null output", "null descriptor array", "src_base must be 16-byte aligned",
            "dst_off must be a multiple of 16", "need f_num < f_den", "object larger than 2^31 blocks"]


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
def want(S, oracle, base):
    """Oracle bytes of one descriptor, computed once and never modified."""
    @functools.lru_cache(maxsize=None)
    def controlled(size, ent, d, c):
        fn, fd = S.compress_ratio(c)
        a = oracle.fill_controlled(size, d, fn, fd, ent, base)
        a.setflags(write=False)
        return a
    return lambda o: controlled(o[1], o[2], o[3], o[4])


def layout(sizes, rnd, gap_blocks=(0,), align=4096, dc=((1, 1),)):
    """tests/test_gpu_batch.py's layout()."""
    objs, off = [], 0
    for j, sz in enumerate(sizes):
        d, c = rnd.choice(dc)
        objs.append((off, sz, P.object_entropy(SEED_BASE, j), d, c))
        off += (sz + align - 1) // align * align + rnd.choice(gap_blocks) * 4096
    return objs, off


def image(objs, end, want, tail=8192):
    """The host buffer: guards everywhere, each object's oracle bytes at its
    offset, and the mask of the bytes that belong to an object."""
    a = np.full(end + tail, GUARD, np.uint8)
    m = np.zeros(end + tail, bool)
    for o in objs:
        if o[1]:
            a[o[0]:o[0] + o[1]] = want(o)
            m[o[0]:o[0] + o[1]] = True
    return a, m


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def judge(S, got, objs, want):
    """What verify_batch must report for the host bytes `got` under descriptors `objs`."""
    per, nbytes, nblocks, first = [], 0, 0, None
    for k, o in enumerate(objs):
        off, size = o[0], o[1]
        if not size:
            continue
        idx = np.flatnonzero(got[off:off + size] != want(o))
        if idx.size == 0:
            continue
        r = S.VerifyResult(int(idx.size), int(np.unique(idx // BLK).size), int(idx.min()))
        per.append((k, r))
        nbytes += r.mismatched_bytes
        nblocks += r.mismatched_blocks
        first = off + r.first_offset if first is None else min(first, off + r.first_offset)
    return S.BatchVerifyResult(S.VerifyResult(nbytes, nblocks, first), len(objs), tuple(per))


def clean(S, n):
    return S.BatchVerifyResult(S.VerifyResult(), n, ())


def flips_expect(S, objs, flips):
    """The result for single `^= 0xFF` bytes at (object index, offset in the
    object) on otherwise clean, non-overlapping objects."""
    by = {}
    for k, p in flips:
        by.setdefault(k, set()).add(p)
    per = tuple((k, S.VerifyResult(len(ps), len({p // BLK for p in ps}), min(ps))) for k, ps in sorted(by.items()))
    tot = S.VerifyResult(sum(r.mismatched_bytes for _, r in per), sum(r.mismatched_blocks for _, r in per),
                         min(objs[k][0] + r.first_offset for k, r in per) if per else None)
    return S.BatchVerifyResult(tot, len(objs), per)


def flip(t, objs, flips):
    for k, p in flips:
        assert 0 <= p < objs[k][1]
        t[objs[k][0] + p] ^= 0xFF


def make_case(case):
    rnd = random.Random(sum(case.encode()))
    if case == "packed20k":
        return layout([20 * KiB + 5] * 600, rnd)
    if case == "gaps":
        return layout([rnd.randint(1, 40 * KiB) for _ in range(600)], rnd, gap_blocks=(0, 0, 1, 3))
    if case == "packed16":
        return layout([rnd.randint(1, 30 * KiB) for _ in range(600)], rnd, align=16)
    if case == "ragged_small":
        return layout([rnd.choice([1, 15, 16, 17, 4095, 4096, 4097, 8191, 12288 + 3]) for _ in range(900)], rnd)
    assert case == "mixed_dc"
    sizes = [rnd.randint(1, 300 * KiB) for _ in range(80)] + [3 * MiB, 3 * MiB - 1, 2 * MiB + 4097, 65 * BLK + 1]
    rnd.shuffle(sizes)
    return layout(sizes, rnd, gap_blocks=(0, 1), dc=((1, 1), (2, 3), (4, 2), (3, (3, 2)), (0, 7)))


CASES = ["packed20k", "gaps", "packed16", "ragged_small", "mixed_dc"]


# ---- 1. clean layouts: every wave count, every tile size, guards changed --------

@pytest.mark.parametrize("case", CASES)
def test_clean_layouts(S, torch, wave_ctx, want, case):
    objs, end = make_case(case)
    a, mask = image(objs, end, want)
    t = dev(torch, a)
    gaps = dev(torch, ~mask)
    for waves, ctx in wave_ctx.items():
        for tile in TILES:
            ctx.set_batch_tile(tile)
            try:
                r = ctx.verify_batch(t, objs)
            finally:
                ctx.set_batch_tile(0)
            assert r == clean(S, len(objs)) and r.ok and r.mismatched_objects == 0, (case, waves, tile, r.total)
    assert np.array_equal(t.cpu().numpy(), a)                 # a read-only pass
    # every gap byte and every byte behind the last object changed: the same result
    t[gaps] = 0x11
    for waves, ctx in wave_ctx.items():
        for tile in (0, 2, 64):
            ctx.set_batch_tile(tile)
            try:
                assert ctx.verify_batch(t, objs) == clean(S, len(objs)), (case, waves, tile)
            finally:
                ctx.set_batch_tile(0)


@pytest.mark.parametrize("variation", ["reversed", "shuffled", "empties", "one_large"])
def test_clean_variations(S, torch, wave_ctx, want, variation):
    rnd = random.Random(7)
    objs, end = layout([rnd.choice([1, 17, 4096, 5000, 12288 + 3, 70000]) for _ in range(500)], rnd,
                       gap_blocks=(0, 1), align=16, dc=((1, 1), (2, 3)))
    if variation == "one_large":
        objs, end = layout([5000] * 20 + [80 * MiB] + [4097] * 20, rnd)
    a, _ = image(objs, end, want)
    t = dev(torch, a)
    if variation == "reversed":
        objs = objs[::-1]
    elif variation == "shuffled":
        rnd.shuffle(objs)
    elif variation == "empties":
        out = []
        for k, o in enumerate(objs):
            out.append(o)
            if k % 3 == 0:                                    # an empty object may say anything else
                out.append((o[0] + 8, 0, 5, 9, 1))
        objs = [(0, 0, 0, 1, 1)] + out + [(end, 0, 0, 1, 1)] * 2
    for waves, ctx in wave_ctx.items():
        for tile in (0, 8, 64):
            ctx.set_batch_tile(tile)
            try:
                assert ctx.verify_batch(t, objs) == clean(S, len(objs)), (variation, waves, tile)
            finally:
                ctx.set_batch_tile(0)
    # one dirty byte in the last object of the buffer: found under its index in this order
    k = max(range(len(objs)), key=lambda j: (objs[j][1] > 0, objs[j][0]))
    fl = [(k, objs[k][1] - 1)]
    flip(t, objs, fl)
    assert wave_ctx[2].verify_batch(t, objs) == flips_expect(S, objs, fl), variation


# ---- 2. one flipped byte at every place the kernel distinguishes ----------------

def flip_layout():
    """16-B packed; index: what it is for."""
    sizes = [3 * BLK + 100,      # 0: first object; compress 2: zero prefix ends at c = 2048 in every block
             1,                  # 1: ragged, 1 byte
             17,                 # 2: ragged, one whole piece and one byte
             0,                  # 3: empty
             70 * BLK + 5,       # 4: right after an empty one; 8-block tiles: 9 tiles, the last with 7 live slots
             2 * BLK,            # 5: compress 1: windows at 0 and 2048
             0, 0,               # 6, 7
             4095,               # 8
             BLK + 16]           # 9: last object
    comp = {0: 2, 5: 1}
    objs, off = [], 0
    for j, sz in enumerate(sizes):
        objs.append((off, sz, P.object_entropy(SEED_BASE + 3, j), 2 if j == 4 else 1, comp.get(j, 3)))
        off += (sz + 15) // 16 * 16
    return objs, off


FLIPS = {
    "first byte of the first object": [(0, 0)],
    "last byte of the first object (ragged block)": [(0, 3 * BLK + 99)],
    "the 1-byte object": [(1, 0)],
    "last byte of the 17-byte object": [(2, 16)],
    "last byte of its whole piece": [(2, 15)],
    "below the zero-prefix end": [(0, BLK + 2047)],
    "at the zero-prefix end": [(0, BLK + 2048)],
    "first byte of the zero prefix": [(0, 2 * BLK)],
    "piece edge, low side": [(4, 5 * BLK + 1023)],
    "piece edge, high side": [(4, 5 * BLK + 1024)],
    "window 1": [(5, 5)],
    "window 1, last byte": [(5, BLK + 31)],
    "window 2": [(5, 2048 + 7)],
    "window 2, last byte": [(5, BLK + 2048 + 31)],
    "block edge, low side": [(4, 3 * BLK - 1)],
    "block edge, high side": [(4, 3 * BLK)],
    "first slot of a tile": [(4, 8 * BLK)],
    "last slot of a full tile": [(4, 8 * BLK - 1)],
    "last live slot of an object's last tile": [(4, 70 * BLK + 4)],
    "first slot of the last tile": [(4, 64 * BLK)],
    "object after an empty one": [(4, 0)],
    "object before empty ones": [(5, 2 * BLK - 1)],
    "first byte of the last object": [(9, 0)],
    "last byte of the last object": [(9, BLK + 15)],
    "two bytes in one block": [(4, 9 * BLK + 7), (4, 9 * BLK + 4000)],
    "two bytes in one piece": [(8, 32), (8, 47)],
    "two bytes in two blocks": [(4, 20 * BLK + 1), (4, 63 * BLK + 4095)],
    "two objects": [(8, 4094), (0, 1)],
}


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_flipped_bytes(S, torch, wave_ctx, want, waves):
    objs, end = flip_layout()
    a, _ = image(objs, end, want)
    t = dev(torch, a)
    ctx = wave_ctx[waves]
    for tile in (8, 0, 2):
        ctx.set_batch_tile(tile)
        try:
            assert ctx.verify_batch(t, objs) == clean(S, len(objs))
            for what, fl in FLIPS.items():
                flip(t, objs, fl)
                r = ctx.verify_batch(t, objs)
                flip(t, objs, fl)                             # back
                assert r == flips_expect(S, objs, fl), (what, tile, r)
                assert r.mismatched_objects == len({k for k, _ in fl}) and not r.ok
            assert ctx.verify_batch(t, objs) == clean(S, len(objs))
        finally:
            ctx.set_batch_tile(0)
    # the judge agrees with the closed form on a mix of all of them
    allf = sorted({f for fl in FLIPS.values() for f in fl})
    flip(t, objs, allf)
    r = ctx.verify_batch(t, objs)
    assert r == flips_expect(S, objs, allf) == judge(S, t.cpu().numpy(), objs, want)


# ---- 3. several dirty objects; the lowest address wins whatever the order --------

@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_every_seventh_object_dirty(S, torch, gpu_ctx, want, order):
    rnd = random.Random(21)
    objs, end = layout([rnd.choice([100, 4096, 9000, 40 * KiB + 1]) for _ in range(300)], rnd, gap_blocks=(0, 1),
                       dc=((1, 1), (2, 2)))
    a, _ = image(objs, end, want)
    for k in range(0, 300, 7):
        for p in {rnd.randrange(objs[k][1]) for _ in range(rnd.randint(1, 5))}:
            a[objs[k][0] + p] ^= 0xFF
    if order == "reversed":
        objs = objs[::-1]                                     # the lowest address is the last descriptor
    t = dev(torch, a)
    r = gpu_ctx.verify_batch(t, objs)
    exp = judge(S, a, objs, want)
    assert r == exp
    assert r.mismatched_objects == 43
    assert r.total.first_offset == min(objs[k][0] + v.first_offset for k, v in r.mismatches)
    if order == "reversed":
        assert r.mismatches[-1][0] == 299 and r.total.first_offset == r.mismatches[-1][1].first_offset


# ---- 4. a wrong descriptor -------------------------------------------------------

@pytest.mark.parametrize("field", ["entropy", "dedup", "compress", "size_down", "size_up"])
def test_wrong_descriptor(S, torch, gpu_ctx, want, field):
    """One object described one step off: only it reports, with the counts of
    the numpy diff of the two oracle outputs."""
    rnd = random.Random(3)
    objs, end = layout([10 * BLK + 77] * 12, rnd, gap_blocks=(1,), dc=((2, 3),))
    a, _ = image(objs, end, want)
    t = dev(torch, a)
    off, size, ent, d, c = objs[5]
    objs[5] = {"entropy": (off, size, ent + 1, d, c), "dedup": (off, size, ent, d + 1, c),
               "compress": (off, size, ent, d, c + 1), "size_down": (off, size - BLK, ent, d, c),
               "size_up": (off, size + BLK - 77, ent, d, c)}[field]      # still inside the one-block gap
    r = gpu_ctx.verify_batch(t, objs)
    exp = judge(S, a, objs, want)
    assert r == exp and [k for k, _ in r.mismatches] == [5]
    assert r.total.mismatched_bytes > 0 and r.total.first_offset == off + r.mismatches[0][1].first_offset


def test_same_region_twice(S, torch, gpu_ctx, want):
    o = (4096, 6 * BLK + 9, 77, 1, 2)
    a, _ = image([o], o[0] + o[1], want)
    t = dev(torch, a)
    objs = [o, (o[0], o[1], 78, 1, 2)]
    r = gpu_ctx.verify_batch(t, objs)
    assert r == judge(S, a, objs, want)
    assert [k for k, _ in r.mismatches] == [1]
    assert (r.total.mismatched_bytes, r.total.mismatched_blocks) == \
        (r.mismatches[0][1].mismatched_bytes, r.mismatches[0][1].mismatched_blocks)
    assert r.total.first_offset == o[0] + r.mismatches[0][1].first_offset
    # both wrong: a byte that is wrong for both counts twice
    twice = gpu_ctx.verify_batch(t, [objs[1], objs[1]])
    assert twice.total.mismatched_bytes == 2 * r.total.mismatched_bytes
    assert twice.total.mismatched_blocks == 2 * r.total.mismatched_blocks
    assert twice.total.first_offset == r.total.first_offset and twice.mismatched_objects == 2


# ---- 5. sub-batch boundaries -------------------------------------------------------

def test_sub_batch_boundaries(S, torch, gpu_ctx, want):
    """50 000 descriptors: sub-batches end at 16 384 and 49 152.  Empties are
    sprinkled in; dirty objects sit on both sides of every cut."""
    rnd = random.Random(50)
    dirty = [0, 16383, 16384, 49151, 49152, 49999]
    sizes = [rnd.choice([1, 4095, 4096, 4097, 12288 + 7, 0]) for _ in range(50000)]
    for k in dirty:
        sizes[k] = sizes[k] or 4097
    objs, end = layout(sizes, rnd, gap_blocks=(0, 0, 1), align=16)
    a, _ = image(objs, end, want)
    t = dev(torch, a)
    assert gpu_ctx.verify_batch(t, objs) == clean(S, 50000)
    fl = [(k, rnd.randrange(objs[k][1])) for k in dirty]
    flip(t, objs, fl)
    for tile in (0, 2):
        gpu_ctx.set_batch_tile(tile)
        try:
            r = gpu_ctx.verify_batch(t, objs)
        finally:
            gpu_ctx.set_batch_tile(0)
        assert r == flips_expect(S, objs, fl), tile
        assert [k for k, _ in r.mismatches] == dirty
    # a first sub-batch of empty objects only
    objs2 = [(0, 0, 0, 1, 1)] * 16384 + objs[:100]
    r = gpu_ctx.verify_batch(t, objs2)
    assert r == flips_expect(S, objs2, [(16384, fl[0][1])])


# ---- 6. a grid above the sub-launch limit ---------------------------------------

def test_grid_above_the_sub_launch_limit(S, torch, gpu_ctx):
    """4100 objects of 4 MiB + 4096 in 64-block tiles: 4 460 800 slots, two
    sub-launches.  Filled by fill_batch (whose bytes are pinned against the
    oracle elsewhere); nothing is copied to the host."""
    n, size = 4100, 4 * MiB + 4096
    slots_per_obj = -(-(size // BLK) // 64) * 64
    assert n * slots_per_obj > MAX_GRID
    objs = [(j * size, size, P.object_entropy(SEED_BASE, j), 1 + j % 2, 1 + j % 3) for j in range(n)]
    t = torch.empty(n * size, dtype=torch.uint8, device="cuda")
    gpu_ctx.set_batch_tile(64)
    try:
        gpu_ctx.fill_batch(t, objs)
        assert gpu_ctx.verify_batch(t, objs) == clean(S, n)
        # slot 2^22 opens the second sub-launch: its object and block, the slot before it, the very last byte
        k, slot = divmod(MAX_GRID, slots_per_obj)
        assert 0 < slot < size // BLK
        fl = [(k, slot * BLK + 5), (k, slot * BLK - 1), (n - 1, size - 1)]
        flip(t, objs, fl)
        assert gpu_ctx.verify_batch(t, objs) == flips_expect(S, objs, fl)
        assert gpu_ctx.verify_batch(t, objs, per_object=False).total == flips_expect(S, objs, fl).total
    finally:
        gpu_ctx.set_batch_tile(0)
        del t


# ---- 7. streams and memory ---------------------------------------------------------

def test_two_threads_two_streams(S, torch, gpu_ctx, want):
    rnd = random.Random(9)
    jobs = []
    for j in range(2):
        objs, end = layout([rnd.choice([17, 4097, 30000, 300 * KiB]) for _ in range(400)], rnd, gap_blocks=(0, 1),
                           dc=((1 + j, 1 + j),))
        a, _ = image(objs, end, want)
        fl = [(k, rnd.randrange(objs[k][1])) for k in rnd.sample(range(400), 5 + j)]
        t = dev(torch, a)
        flip(t, objs, fl)
        jobs.append((objs, t, flips_expect(S, objs, fl), torch.cuda.Stream()))
    torch.cuda.synchronize()
    got, errs = {}, []

    def work(j):
        objs, t, _, s = jobs[j]
        try:
            got[j] = [gpu_ctx.verify_batch(t, objs, stream=s) for _ in range(20)]
        except Exception as e:                                # noqa: BLE001
            errs.append(repr(e))
    ts = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    [x.start() for x in ts]
    [x.join() for x in ts]
    assert not errs, errs
    for j in range(2):
        assert all(r == jobs[j][2] for r in got[j]), j
        gpu_ctx.release_stream(jobs[j][3])


def test_repeated_calls_do_not_grow_device_memory(S, torch, want):
    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    rnd = random.Random(13)
    objs, end = layout([rnd.choice([1, 5000, 70000]) for _ in range(3000)], rnd)
    a, _ = image(objs, end, want)
    t = dev(torch, a)
    fl = [(7, 0), (2999, 0)]
    flip(t, objs, fl)
    s = torch.cuda.Stream()

    def dev_used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    def round_():
        for _ in range(50):
            assert ctx.verify_batch(t, objs, stream=s) == flips_expect(S, objs, fl)
            assert ctx.verify_batch(t, objs[:10]) == flips_expect(S, objs[:10], fl[:1])
    round_()
    d0 = dev_used()
    round_()
    assert dev_used() <= d0, "device memory grew across repeated verify_batch calls"
    ctx.release_stream(s)
    assert dev_used() <= d0
    ctx.close()


# ---- 8. totals only ----------------------------------------------------------------

def test_totals_only(S, torch, gpu_ctx, want):
    rnd = random.Random(17)
    objs, end = layout([rnd.randint(1, 50000) for _ in range(200)], rnd, align=16)
    a, _ = image(objs, end, want)
    t = dev(torch, a)
    r = gpu_ctx.verify_batch(t, objs, per_object=False)
    assert r == S.BatchVerifyResult(S.VerifyResult(), 200, None) and r.ok and r.mismatched_objects is None
    fl = sorted({(k, rnd.randrange(objs[k][1])) for k in (3, 3, 77, 199)})
    flip(t, objs, fl)
    full = gpu_ctx.verify_batch(t, objs)
    r = gpu_ctx.verify_batch(t, objs, per_object=False)
    assert full == flips_expect(S, objs, fl)
    assert r.total == full.total and r.mismatches is None and r.objects == 200 and not r.ok
    # the C call with per_obj == NULL, and an empty batch
    from s3dlio_amd import _lib
    arr = (_lib.ObjDesc * 200)(*[_lib.ObjDesc(o[0], o[1], o[2], o[3], *S.compress_ratio(o[4])) for o in objs])
    tot = _lib.VerifyRec()
    _lib.call("s3dg_verify_controlled_batch", gpu_ctx._h, t.data_ptr(), arr, 200, 0, ctypes.byref(tot), None)
    assert S.VerifyResult._of(tot) == full.total
    assert gpu_ctx.verify_batch(t, []) == clean(S, 0)
    assert gpu_ctx.verify_batch(t, [(8, 0, 1, 1, 1)] * 3) == clean(S, 3)   # all empty: nothing is launched


# ---- 9. refusals ------------------------------------------------------------------

def test_refusals(S, torch, gpu_ctx, want):
    """Every refusal of the contract with its message; nothing is reported and
    the buffer is untouched."""
    from s3dlio_amd import _lib
    D = _lib.ObjDesc
    objs, end = layout([5000] * 4, random.Random(1))
    a, _ = image(objs, end, want)
    a[10] ^= 0xFF                                             # a dirty byte a launch would report
    t = dev(torch, a)
    good = [D(o[0], o[1], o[2], o[3], 0, 1) for o in objs]
    p = t.data_ptr()

    def refused(msg, src, descs, n, out=True, per=True):
        arr = (D * max(1, len(descs)))(*descs) if descs is not None else None
        tot, rec = _lib.VerifyRec(), (_lib.VerifyRec * 8)()
        ctypes.memset(ctypes.byref(tot), 0x5A, ctypes.sizeof(tot))
        ctypes.memset(rec, 0x5A, ctypes.sizeof(rec))
        with pytest.raises(ValueError) as ei:
            _lib.call("s3dg_verify_controlled_batch", gpu_ctx._h, src, arr, n, 0,
                      ctypes.byref(tot) if out else None, rec if per else None)
        assert msg in str(ei.value), (msg, str(ei.value))
        assert bytes(tot) == b"\x5a" * 24 and bytes(rec) == b"\x5a" * 192      # written only on success

    refused(REFUSALS[0], p, good, 4, out=False)
    refused(REFUSALS[0], p, good, 0, out=False)
    refused(REFUSALS[1], p, None, 4)
    refused(REFUSALS[2], None, good, 4)
    refused(REFUSALS[2], p + 8, good, 4)
    bad = {REFUSALS[3]: D(8, 100, 1, 1, 0, 1), REFUSALS[4]: D(0, 100, 1, 1, 3, 3),
           REFUSALS[5]: D(0, (1 << 31) * BLK, 1, 1, 0, 1)}
    for msg, b in bad.items():
        for at in range(4):                                   # the first descriptor, the last, in between
            refused(msg, p, good[:at] + [b] + good[at + 1:], 4)
    refused(REFUSALS[4], p, good[:3] + [D(0, 100, 1, 1, 0, 0)], 4)             # f_den == 0: the random-data layout
    refused(REFUSALS[3], p, good[:1] + [bad[REFUSALS[3]], bad[REFUSALS[4]]] + good[3:], 4)   # the first one names it
    refused(REFUSALS[4], p, good[:1] + [bad[REFUSALS[4]], bad[REFUSALS[3]]] + good[3:], 4)
    # a bad descriptor far behind the first sub-batch: still nothing has run
    many = good * 5000 + [bad[REFUSALS[4]]]
    refused(REFUSALS[4], p, many, len(many), per=False)
    # the Python method: bounds against the tensor before any launch
    with pytest.raises(ValueError, match="reads"):
        gpu_ctx.verify_batch(t, objs + [(end + 8192 - 100, 101, 1, 1, 1)])
    with pytest.raises(ValueError, match="multiple of 16"):
        gpu_ctx.verify_batch(t, [objs[0], (8, 100, 2, 1, 1)])
    assert np.array_equal(t.cpu().numpy(), a)
    assert gpu_ctx.verify_batch(t, objs) == flips_expect(S, objs, [(0, 10)])   # and the context still works


# ---- 10. one moderate end-to-end case -------------------------------------------

def test_fill_then_verify_end_to_end(S, torch, gpu_ctx):
    """600 log-uniform sizes (4 KiB .. 4 MiB), two (d, c) pairs: fill_batch then
    verify_batch is clean; after 20 seeded flips the result is numpy's."""
    rnd = random.Random(4)
    sizes = [int(math.exp(rnd.uniform(math.log(4096), math.log(4 * MiB)))) for _ in range(600)]
    objs, end = layout(sizes, rnd, dc=((2, (3, 2)), (1, 1)))
    t = torch.full((end + 8192,), GUARD, dtype=torch.uint8, device="cuda")
    gpu_ctx.fill_batch(t, objs)
    assert gpu_ctx.verify_batch(t, objs) == clean(S, 600)
    before = t.cpu().numpy()
    fl = []
    for _ in range(20):
        k = rnd.randrange(600)
        fl.append((k, rnd.randrange(objs[k][1])))
    fl = sorted(set(fl))
    flip(t, objs, fl)
    r = gpu_ctx.verify_batch(t, objs)
    assert r == judge(S, t.cpu().numpy(), objs, lambda o: before[o[0]:o[0] + o[1]])
    assert r == flips_expect(S, objs, fl)
