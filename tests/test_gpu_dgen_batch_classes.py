"""GPU: the DG1 batch (k_keystream_batch, k_verify_keystream_batch) at every
size class, lane edge and shared wave, over the lists of
tests/dgen_batch_cases.py.  Those builders assert from a restatement of the
plan (held against the header in tests/test_dgen_batch_cpu.py) that their
lists reach what they are built for; here the lists run.

Expected bytes come only from the C oracle (oracle_c.dgen_fill), expected
verify results only from numpy (tests/test_gpu_dgen_batch.py's `expect`), and
every comparison is exact.  Buffers are poisoned and compared whole.

  * class lengths: every ragged class 0..8 at each min_lane_draws knob, with
    tails at the class's edges and 17 bytes to either side of three lane
    boundaries (a region that ends on, just below or just above a lane's end,
    the 1-7 byte tail draw as a lane's first or last, whole lanes empty),
    behind 0, 1 and 2 full blocks; at 32 KiB and 4 KiB lanes also at every
    stage width in 1- and 4-wave workgroups.  Then every object in a call of
    its own, where no neighbour in the wave can take the masked path for it.
  * prefix ends: a zero prefix that ends at every residue mod 16 in the last
    stage of one lane and in the first stage of the next, filled, verified and
    with a flipped bit on either side of the prefix's end.
  * all ten classes in one call, launches with and without zero prefixes.
  * attribution in a shared wave: 64 / lpc objects in one wave of the verify
    (2 .. 64 objects, rows of two objects in one ballot), with differences in
    every object at once, in neighbouring objects, in last bytes beside
    inverted gaps, over the granules of one object, over a whole object and at
    random: each object gets its own bytes, granules and first offset.
  * 20 000 objects of 1 .. 80 bytes: record tables and the per-object array
    regrow, remapped workgroup groups followed by a partial one, then calls of
    6 500, 3 and 20 000 objects on the same stream.

The default knob (2048, "not set") runs the 4 KiB-lane lists; what lanes it
gives them depends on the device, so nothing is claimed for it but the bytes.
"""
import functools

import numpy as np
import pytest

import dgen_batch_cases as K
from test_gpu_dgen_batch import KNOBS, S, clean, ctxs, expect, filled, poisoned, torch, want_of  # noqa: F401

pytestmark = pytest.mark.gpu

MIB = K.MIB
SHAPE_KNOBS = (512, 4096)          # lanes shorter than most chunks: every stage width and workgroup shape too


@pytest.fixture
def dgen(S, oracle):
    """Oracle bytes, computed once per argument set within a test and never modified."""
    @functools.lru_cache(maxsize=None)
    def f(size, dedup, compress, seed):
        fn, fd = S.compress_ratio(compress)
        a = oracle.dgen_fill(size, dedup, fn, fd, seed)
        a.setflags(write=False)
        return a
    return f


def filled_at_every_shape(torch, S, dgen, ctx, knob, objs, total):
    """filled(), then at the knobs of SHAPE_KNOBS the same bytes at draws
    16/32/64 in 1- and 4-wave workgroups.  Returns (tensor, want)."""
    t, want = filled(torch, S, dgen, ctx, objs, total)
    if knob in SHAPE_KNOBS:
        want_dev = torch.from_numpy(want).to("cuda:0")
        try:
            for draws in (16, 32, 64):
                for waves in (1, 4):
                    ctx.set_keystream_shape(1, draws=draws, waves=waves, min_lane_draws=knob)
                    u = poisoned(torch, total)
                    ctx.dgen_fill_batch(u, objs)
                    assert torch.equal(u, want_dev), (knob, draws, waves)
                    assert ctx.verify_dgen_batch(u, objs, per_object=False) == clean(S, len(objs), False)
        finally:
            ctx.set_keystream_shape(1, min_lane_draws=knob)
    return t, want


# ---- 1. lengths around the lane boundaries of every class ---------------------------------------

@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("cls", K.RAGGED)
def test_class_lengths(S, torch, ctxs, dgen, cls, knob):
    """The list in one call, then every object in a call of its own.  A stage
    takes the masked path for the whole wave as soon as one lane is at its
    1-4 byte tail draw, so in the one call a neighbour's tail can cover for a
    lane that missed its own; alone in its wave a lane has no such help."""
    ctx = ctxs[knob]
    objs, total = K.class_lengths(cls, K.list_knob(knob))
    t, want = filled_at_every_shape(torch, S, dgen, ctx, knob, objs, total)
    u = poisoned(torch, total)
    for o in objs:
        ctx.dgen_fill_batch(u, [o])
    assert np.array_equal(u.cpu().numpy(), want)
    for o in objs:
        assert ctx.verify_dgen_batch(t, [o], per_object=False) == clean(S, 1, False), o


# ---- 2. zero prefixes that end next to a lane start -------------------------------------------------

@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("cls", K.RAGGED[1:])
def test_prefix_ends(S, torch, ctxs, dgen, cls, knob):
    """Filled and verified as the class lengths; then one flipped bit in the
    prefix's last byte and in the first byte behind it, apart and together,
    for the objects whose prefix ends 1 byte below, 1 byte above and 16 bytes
    above the boundary."""
    ctx = ctxs[knob]
    objs, total = K.prefix_ends(cls, K.list_knob(knob))
    t, want = filled_at_every_shape(torch, S, dgen, ctx, knob, objs, total)
    b = K.prefix_boundary(cls, K.list_knob(knob))
    got = want.copy()
    for z in (b - 1, b + 1, b + 16):
        k = next(i for i, o in enumerate(objs) if K.tail_of(o)[2] == z)
        p, ln, zlen = K.tail_of(objs[k])
        assert 0 < zlen < ln and not want[p:p + zlen].any()
        for sites in ((p + zlen - 1,), (p + zlen,), (p + zlen - 1, p + zlen)):
            for q in sites:
                t[q] ^= 0x02
                got[q] ^= 0x02
            r = ctx.verify_dgen_batch(t, objs)
            assert r == expect(S, dgen, objs, got), (cls, knob, z, sites)
            assert r.total.mismatched_bytes == len(sites) and [i for i, _ in r.mismatches] == [k]
            for q in sites:
                t[q] ^= 0x02
                got[q] ^= 0x02
    assert np.array_equal(t.cpu().numpy(), want)


# ---- 3. every class in one call ------------------------------------------------------------------------

def test_all_classes_in_one_call(S, torch, gpu_ctx, dgen):
    objs, total = K.all_classes()
    t, want = filled(torch, S, dgen, gpu_ctx, objs, total)
    gpu_ctx.dgen_fill_batch(t, objs[::-1])                      # again, in reverse order
    assert np.array_equal(t.cpu().numpy(), want)
    assert gpu_ctx.verify_dgen_batch(t, objs[::-1]) == clean(S, len(objs))
    got = want.copy()
    hit = {}
    for k, o in enumerate(objs):                                # one object per class, in its last chunk
        hit.setdefault(K.class_of_object(o), k)
    assert sorted(hit) == list(range(K.FULL + 1))
    for cls, k in hit.items():
        off, size = objs[k][0], objs[k][1]
        tail = size % MIB or MIB
        got[off + size - tail + (tail * 5 // 7)] ^= 0x20
    t = torch.from_numpy(got).to("cuda:0")
    e = expect(S, dgen, objs, got)
    assert e.total.mismatched_bytes == K.FULL + 1 and sorted(i for i, _ in e.mismatches) == sorted(hit.values())
    assert gpu_ctx.verify_dgen_batch(t, objs) == e
    assert gpu_ctx.verify_dgen_batch(t, objs, per_object=False) == expect(S, dgen, objs, got, False)
    assert np.array_equal(t.cpu().numpy(), got)                 # nothing is written


# ---- 4. attribution where a wave holds several objects ------------------------------------------------------

def expect_sparse(S, dgen, objs, got, sites):
    """expect() for a `got` that is the oracle's everywhere but at `sites`
    (buffer offsets): the objects that hold no site are clean by construction
    and are handed to expect() as empty, so only the others are compared."""
    sites = np.sort(np.asarray(sites))
    masked = []
    for o in objs:
        lo, hi = np.searchsorted(sites, (o[0], o[0] + o[1]))
        masked.append(o if hi > lo else (o[0], 0) + tuple(o[2:]))
    return expect(S, dgen, masked, got)


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("cls", K.RAGGED)
def test_shared_wave_attribution(S, torch, ctxs, dgen, cls, knob):
    """Six corruption patterns on a clean device copy of the oracle bytes, each
    its own verify call: totals and per-object results are numpy's."""
    ctx = ctxs[knob]
    objs, total = K.shared_wave(cls, K.list_knob(knob))
    n = len(objs)
    want = want_of(dgen, objs, total)
    got = want.copy()
    t = torch.from_numpy(want).to("cuda:0")
    tails = [K.tail_of(o) for o in objs]                        # (offset in the buffer, len, zlen)
    minlen = min(ln for _p, ln, _z in tails)
    p1 = (minlen - 1) // K.STAGE * K.STAGE - K.STAGE + 200     # the same stage and piece of every tail
    p2 = p1 + 48                                                # another 16-byte piece of that stage
    assert 0 <= p1 < p2 < minlen and p1 // K.STAGE == p2 // K.STAGE and p1 // 16 != p2 // 16
    assert ctx.verify_dgen_batch(t, objs) == clean(S, n)

    def run(sites, what, full=False, unwritten=True):
        """XORs the (offset, mask) sites into both copies, verifies, restores.
        (The many pair calls skip the second verify and the read-back: at one
        lane per chunk a full block in the list costs each call ~10 ms.)"""
        if isinstance(sites, list):
            sites = (np.array([p for p, _ in sites], np.int64), np.array([m for _, m in sites], np.uint8))
        where, mask = sites
        assert np.unique(where).size == where.size and mask.all()
        idx, msk = torch.from_numpy(where).to("cuda:0"), torch.from_numpy(mask).to("cuda:0")
        t[idx] ^= msk
        got[where] ^= mask
        e = expect(S, dgen, objs, got) if full else expect_sparse(S, dgen, objs, got, where)
        r = ctx.verify_dgen_batch(t, objs)
        assert r == e, (cls, knob, what)
        if unwritten:                                           # the totals alone; and nothing is written
            assert ctx.verify_dgen_batch(t, objs, per_object=False) == type(e)(e.total, n, None), (cls, knob, what)
            assert np.array_equal(t.cpu().numpy(), got), what
        t[idx] ^= msk
        got[where] ^= mask
        return e

    # 1. every object, the same offset within the tail
    e = run([(p + p1, 0x01) for p, _ln, _z in tails], "every object", full=True)
    assert e.total.mismatched_bytes == n and e.mismatched_objects == n
    # 2. neighbours in the class's record order (the descriptors'), in the first wave and across its end
    for k in range(min(max(K.wave_objects(cls, K.list_knob(knob)), 4), n - 1)):
        a, b = tails[k][0], tails[k + 1][0]
        e = run([(a + p1, 0x80), (b + p1, 0x80)], ("pair, same offset", k), unwritten=False)
        assert [i for i, _ in e.mismatches] == [k, k + 1]
        e = run([(a + p1, 0x04), (b + p2, 0x04)], ("pair, two pieces", k), unwritten=False)
        assert [i for i, _ in e.mismatches] == [k, k + 1]
    # 3. the last byte of every second object, and every gap byte up to the next multiple of 16 inverted
    sites = [(o[0] + o[1] - 1, 0x40) for o in objs[::2]]
    for o in objs:
        end = o[0] + o[1]
        sites += [(q, 0xFF) for q in range(end, (end + 15) // 16 * 16)]
    nobj = len(objs[::2])
    e = run(sites, "last bytes and gaps")
    assert e.total.mismatched_bytes == nobj and [i for i, _ in e.mismatches] == list(range(0, n, 2))
    # 4. one object with full blocks in front: bytes in several granules of its tail only
    k = next(i for i, o in enumerate(objs) if o[1] > MIB)
    off, size = objs[k][0], objs[k][1]
    p, ln, _z = tails[k]
    ngran = -(-ln // 4096)
    grans = sorted(set(range(ngran)) if ngran <= 16 else {g * (ngran - 1) // 15 for g in range(16)})
    sites = [(p + min(g * 4096 + (37 * g + 5) % 4096, ln - 1), 0x08) for g in grans]
    sites.append((sites[(len(sites) - 1) // 2][0] ^ 1, 0x08))   # a second byte in one of those granules
    e = run(sites, "granules of one tail", full=True)
    assert e.mismatches == ((k, S.VerifyResult(len(grans) + 1, len(grans), min(q for q, _ in sites) - off)),)
    # 5. that object complemented whole: full blocks and tail
    e = run((np.arange(off, off + size), np.full(size, 0xFF, np.uint8)), "a whole object")
    assert e.mismatches == ((k, S.VerifyResult(size, -(-size // 4096), 0)),)
    # 6. about 1 % of the bytes, at random
    rng = np.random.default_rng(0xBAD + 16 * cls + knob)
    where = np.unique(rng.integers(0, total, size=total // 100))
    e = run((where, rng.integers(1, 256, size=where.size).astype(np.uint8)), "random", full=True)
    assert e.mismatched_objects > n // 2 and e.total.mismatched_bytes > total // 400
    assert np.array_equal(t.cpu().numpy(), want)


# ---- 5. large calls ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zeros", [True, False], ids=["zeros", "c1"])
def test_many_tiny_objects(S, torch, gpu_ctx, dgen, zeros):
    """20 000 objects in one call, one oracle call per object, after a small
    call has sized the stream's tables: fill, verify clean and dirty, then 6 500,
    3 and 20 000 objects on the same stream, each compared whole."""
    small, stotal = K.many_tiny(2, zeros)
    filled(torch, S, dgen, gpu_ctx, small, stotal)
    objs, total = K.many_tiny(20000, zeros)
    n = len(objs)
    t, want = filled(torch, S, dgen, gpu_ctx, objs, total)
    got = want.copy()
    dirty = sorted({0, 1023, 1024, 4095, 4096, n - 1} | set(range(0, n, 997)))
    for k in dirty:
        off, size = objs[k][0], objs[k][1]
        got[off + (k % size)] ^= 0x01
        if size > 40:
            got[off + size - 1] ^= 0x80
    t = torch.from_numpy(got).to("cuda:0")
    e = expect(S, dgen, objs, got)
    assert [i for i, _ in e.mismatches] == dirty
    assert gpu_ctx.verify_dgen_batch(t, objs) == e
    assert gpu_ctx.verify_dgen_batch(t, objs, per_object=False) == expect(S, dgen, objs, got, False)
    assert np.array_equal(t.cpu().numpy(), got)
    for m in (6500, 3, 20000):
        filled(torch, S, dgen, gpu_ctx, *K.many_tiny(m, zeros))
