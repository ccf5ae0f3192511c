"""Descriptor lists for the DG1 batch, aimed at the places
where its launches can go wrong, and a plain restatement of the call's lane
plan (csrc/s3dg_dgen_batch_plan.h) that says where those places are.  No torch,
no GPU: tests/test_dgen_batch_cpu.py holds the restatement against the header
line by line and calls every builder, so each builder's own coverage
assertions run in the CPU suite; tests/test_gpu_dgen_batch_classes.py runs the
lists on a device.  Not a conftest.

A list is (objects, buffer bytes) with objects (off, size, seed, dedup,
compress) as Context.dgen_fill_batch takes them, laid out by `layout`: offsets
that are multiples of 16 and not of 4096, gaps of 16 to 4112 bytes, a seed per
object, shuffled.

The builders target the three min_lane_draws knobs at which lanes do not depend
on the device: 131072, 4096 and 512 draws, i.e. lanes of the class's ceiling C,
of 32 KiB and of 4 KiB (lpc = max(1, C / 8 / knob) lanes per chunk, for the
fill and the verify alike).  The default knob reuses the lists of `list_knob`
without a coverage claim.
"""
from __future__ import annotations

import functools
import random
from fractions import Fraction

MIB = 1 << 20
KNOBS = (131072, 4096, 512)
FULL = 9                          # kDgbFull: the class of full 1 MiB chunks
RAGGED = tuple(range(FULL))       # ceilings 4 KiB << cls
COMPRESS = (1, 2, 3, (3, 2))
DEDUPS = (1, 2, 3)
DELTAS = (-17, -16, -15, -9, -8, -7, -5, -4, -1, 0, 1, 4, 5, 7, 8, 9, 15, 16, 17)
BUDGET = 64 * MIB                 # object bytes of one list: bounds the oracle's work
STAGE = 512                       # bytes of a 64-draw stage, the verify's; the fill's are 128, 256 or 512
MIN_STAGE = 128
CUS = 256                         # compute units assumed where the default rule asks


# ---- the plan, restated from the header's comments ---------------------------------------

def chunk_class(length: int) -> int:
    """FULL for a full block, else the smallest k with length <= 4 KiB << k."""
    if length >= MIB:
        return FULL
    k = 0
    while (4096 << k) < length:
        k += 1
    return k


def class_ceiling(cls: int) -> int:
    """Bytes a class is planned for."""
    return MIB if cls >= FULL else 4096 << cls


def _ceil_to(x: int, m: int) -> int:
    return -(-x // m) * m


def _lanes(nd, nchunks, cus, min_draws, spread_floor, max_lpc=1024):
    """Lanes of at least min_draws draws; with spread_floor, a launch of few
    chunks is spread further, down to that many draws, to about 4 waves per CU."""
    lpc = 1
    while lpc < max_lpc and nd // (2 * lpc) >= min_draws:
        lpc *= 2
    if spread_floor:
        while lpc < max_lpc and nchunks * lpc < cus * 4 * 64 and nd // (2 * lpc) >= spread_floor:
            lpc *= 2
    return lpc


def class_lanes(ceil_bytes: int, nchunks: int, cus: int, knob: int, zeros: bool, draws: int, verify: bool):
    """(lpc, span) of a launch planned for chunks of ceil_bytes.
    fill: lanes of at least `knob` draws (not set: 2048, or 512 when the launch
    has zero prefixes, and then spread down to 256); span a multiple of `draws`.
    verify: the knob (not set: 512 when the launch has zero prefixes, which
    counts as set; else 2048, spread down to 512) rounded up to whole granules
    of 512 draws; span a multiple of 512."""
    nd = ceil_bytes // 8
    if verify:
        k = knob or (512 if zeros else 0)
        lpc = _lanes(nd, nchunks, cus, _ceil_to(k or 2048, 512), 0 if k else 512)
        return lpc, _ceil_to(-(-nd // lpc), 512)
    lpc = _lanes(nd, nchunks, cus, knob or (512 if zeros else 2048), 0 if knob else 256)
    return lpc, _ceil_to(-(-nd // lpc), draws)


def lane_region(length: int, span: int, sub: int):
    """(rb, rlen) of lane `sub` of a chunk of `length` bytes; rlen 0: nothing."""
    rb = sub * span * 8
    return rb, max(0, min(length - rb, span * 8))


def ratio(compress):
    """(f_num, f_den) of a compress value, as s3dlio_amd.compress_ratio."""
    if isinstance(compress, int):
        return (compress - 1, compress) if compress > 1 else (0, 1)
    fr = Fraction(*compress) if isinstance(compress, tuple) else Fraction(compress).limit_denominator(1 << 16)
    return (0, 1) if fr <= 1 else (fr.numerator - fr.denominator, fr.numerator)


def chunks(objs):
    """The call's records as (object index, block, len, zlen), in the descriptors' order."""
    for k, (_off, size, _seed, _dd, comp) in enumerate(objs):
        fn, fd = ratio(comp)
        nb = -(-size // MIB)
        for i in range(nb):
            ln = MIB if i + 1 < nb or size % MIB == 0 else size % MIB
            yield k, i, ln, ln * fn // fd


def class_counts(objs):
    """(chunks, chunks with a zero prefix) per class: what decides the call's launches."""
    count, zeros = [0] * (FULL + 1), [0] * (FULL + 1)
    for _k, _i, ln, z in chunks(objs):
        count[chunk_class(ln)] += 1
        zeros[chunk_class(ln)] += z != 0
    return count, zeros


def tail_of(obj):
    """(offset of the ragged last chunk in the buffer, its len, its zlen)."""
    off, size, _seed, _dd, comp = obj
    ln = size % MIB
    fn, fd = ratio(comp)
    return off + size - ln, ln, ln * fn // fd


def object_bytes(objs) -> int:
    return sum(o[1] for o in objs)


def knob_lanes(cls: int, knob: int):
    """(lpc, lane bytes) of a class at one of KNOBS: the same for the fill at
    every stage width, for the verify, with and without zero prefixes and
    whatever the launch's size."""
    C = class_ceiling(cls)
    lpc = max(1, C // 8 // knob)
    for zeros in (False, True):
        for n in (1, 67, 20000):
            for draws in (16, 32, 64):
                assert class_lanes(C, n, CUS, knob, zeros, draws, False) == (lpc, C // 8 // lpc)
            assert class_lanes(C, n, CUS, knob, zeros, 64, True) == (lpc, C // 8 // lpc)
    return lpc, C // lpc


def list_knob(knob: int) -> int:
    """The knob whose lists a context at `knob` runs: its own, or for the
    default (which spreads these small launches to the shortest lanes) 512."""
    return knob if knob in KNOBS else 512


# ---- layout -------------------------------------------------------------------------------

def layout(sizes, params, seed0, rng):
    """(off, size, seed, dedup, compress) per size: offsets that are multiples
    of 16 and not of 4096, gaps of 16 to 4112 bytes, a seed per object;
    params(k) -> (dedup, compress).  Returns (objects, buffer bytes)."""
    objs, end = [], 0
    for k, size in enumerate(sizes):
        off = (end + 15) // 16 * 16 + 16 * rng.randint(1, 257)
        if off % 4096 == 0:
            off += 16
        dd, comp = params(k)
        objs.append((off, size, seed0 + 1000003 * k, dd, comp))
        end = max(end, off + size)
    return objs, (end + 15) // 16 * 16 + 4112


def _list(items, seed0, shuffle=True):
    """items: (size, dedup, compress), shuffled and laid out."""
    rng = random.Random(seed0)
    items = list(items)
    if shuffle:
        rng.shuffle(items)
    objs, total = layout([i[0] for i in items], lambda k: (items[k][1], items[k][2]), seed0, rng)
    assert all(o[0] % 16 == 0 and o[0] % 4096 for o in objs) and len({o[2] for o in objs}) == len(objs)
    assert object_bytes(objs) <= BUDGET, (object_bytes(objs), len(objs))
    return objs, total


def _lo(cls):
    return 0 if cls == 0 else class_ceiling(cls) // 2


def _hi(cls):
    """The longest chunk of a ragged class: its ceiling, but 1 MiB is a full block."""
    return min(class_ceiling(cls), MIB - 1)


def _ragged(objs, cls):
    """The lens of the list's ragged chunks, all of which must be of class cls."""
    lens = [ln for _k, _i, ln, _z in chunks(objs) if ln < MIB]
    assert lens and all(chunk_class(ln) == cls and _lo(cls) < ln <= _hi(cls) for ln in lens)
    return lens


# ---- 1. every length at which a lane's region changes shape ---------------------------------

def boundaries(cls: int, knob: int):
    """Three lane boundaries of the class at the knob: the first above C/2, one
    in the middle and the last, (lpc - 1) lanes; C itself, the last lane's end,
    counts as one.  With one lane per chunk: stage boundaries instead."""
    C, lo = class_ceiling(cls), _lo(cls)
    lpc, lane = knob_lanes(cls, knob)
    if lpc == 1:
        return [lo + STAGE, (lo + C) // 2 // STAGE * STAGE, C - STAGE]
    cand = [k * lane for k in range(1, lpc + 1) if k * lane > lo]
    out = []
    for b in (cand[0], cand[len(cand) // 2], (lpc - 1) * lane):
        if b not in out:
            out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def class_lengths(cls: int, knob: int):
    """Tails C/2 + 1, C - 1, C and b + DELTAS around three boundaries, behind 0,
    1 and 2 full blocks, compress and dedup cycling (a tail of 1 MiB would be a
    full block: the 1 MiB class ends at C - 1).  Where the list would pass
    the byte budget it keeps fewer boundaries (the first and the last, then the
    last), never fewer deltas."""
    C, lo, hi = class_ceiling(cls), _lo(cls), _hi(cls)
    lpc, lane = knob_lanes(cls, knob)
    bs = boundaries(cls, knob)
    for keep in (bs, [bs[0], bs[-1]], [bs[-1]]):
        lens = sorted({lo + 1, C - 1, hi} | {b + d for b in keep for d in DELTAS if lo < b + d <= hi})
        items = [(MIB * (i % 3) + ln, DEDUPS[(i + i // 3) % 3], COMPRESS[i % 4]) for i, ln in enumerate(lens)]
        if sum(i[0] for i in items) <= BUDGET:
            break
    objs, total = _list(items, 0xC1A55 + 131 * cls + knob)
    got = _ragged(objs, cls)
    assert sorted(got) == lens and all(b + d in lens for b in keep for d in DELTAS if lo < b + d <= hi)
    count, _ = class_counts(objs)
    assert count[cls] == len(lens) and count[FULL] > 0                    # the full launch shares the objects
    assert {o[1] // MIB for o in objs} == {0, 1, 2}
    if lpc > 1:
        span = lane // 8
        into, below, empty, exact = set(), set(), False, False
        for ln in lens:
            regions = [lane_region(ln, span, s) for s in range(lpc)]
            assert sum(r[1] for r in regions) == ln
            rlen = [r[1] for r in regions if r[1]][-1]                    # the last lane that has bytes
            exact |= rlen == lane
            if 1 <= rlen <= 7:
                into.add(1 <= (ln & 7) <= 4)
            if 1 <= lane - rlen <= 7:
                below.add(1 <= (ln & 7) <= 4)
            empty |= regions[-1][1] == 0
        assert exact, "no chunk ends on a lane boundary"
        assert into == {True, False}, "tails of 1-4 and of 5-7 bytes at a lane's start"
        assert below == {True, False}, "tails of 1-4 and of 5-7 bytes at a lane's end"
        # with two lanes every chunk of the class (len > C/2) reaches the second
        assert empty or lpc == 2, "no chunk leaves a lane empty"
    return objs, total


# ---- 2. a zero prefix that ends at every residue next to a lane start --------------------------

def prefix_boundary(cls: int, knob: int) -> int:
    """The lane boundary nearest 3C/8 inside [C/4 + 32, C/2]; C/2 where it is
    the only one; with one lane the stage boundary 3C/8."""
    C = class_ceiling(cls)
    lpc, lane = knob_lanes(cls, knob)
    if lpc == 1:
        return 3 * C // 8
    cand = [k * lane for k in range(1, lpc) if C // 4 + 32 <= k * lane <= C // 2]
    return min(cand, key=lambda b: abs(b - 3 * C // 8))


@functools.lru_cache(maxsize=None)
def prefix_ends(cls: int, knob: int):
    """Compress 2 with zlen = len // 2 at every value b - 17 .. min(b + 17, C/2),
    len even and odd in turn; then compress 3 with zlen = 2 len // 3 at
    b + 1 .. b + 16.  Every eighth object has a full block in front."""
    assert cls >= 1
    C = class_ceiling(cls)
    lpc, lane = knob_lanes(cls, knob)
    b = prefix_boundary(cls, knob)
    assert b % (lane if lpc > 1 else STAGE) == 0 and C // 4 + 32 <= b <= C // 2
    want = []                                                             # (len, compress, zlen)
    for i, z in enumerate(range(b - 17, min(b + 17, _hi(cls) // 2) + 1)):
        ln = 2 * z + (i & 1)
        want.append((ln if ln <= _hi(cls) else 2 * z, 2, z))
    for z in range(b + 1, b + 17):
        want.append(((3 * z + 1) // 2, 3, z))
    items = [(ln + (MIB if i % 8 == 3 else 0), 1, comp) for i, (ln, comp, _z) in enumerate(want)]
    objs, total = _list(items, 0x9EF1 + 131 * cls + knob)
    _ragged(objs, cls)
    assert sorted(tail_of(o)[1:] for o in objs) == sorted((ln, z) for ln, _c, z in want)
    assert {tail_of(o)[1] & 1 for o in objs if o[4] == 2} == {0, 1}
    # the prefix ends inside the last stage of the lane that ends at b, or inside
    # the first stage of the lane that starts there, at every stage width
    ends, starts = set(), set()
    for o in objs:
        _p, ln, z = tail_of(o)
        if b - MIN_STAGE < z < b:
            ends.add(z % 16)
        if b < z < b + MIN_STAGE and z < ln:
            starts.add(z % 16)
    assert ends == set(range(16)) and starts == set(range(16)), (sorted(ends), sorted(starts))
    return objs, total


# ---- 3. every class in one call ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_classes():
    """Tails C/2 + 17 and C - 1 of every ragged class, some behind full blocks,
    and objects of whole blocks.  Even classes hold compress 1 only, so the call
    has launches with and without zero prefixes."""
    items = []
    for cls in RAGGED:
        C = class_ceiling(cls)
        for j, ln in enumerate((_lo(cls) + 17, C - 1)):
            comp = 1 if cls % 2 == 0 else COMPRESS[1 + (cls // 2 + j) % 3]
            items.append((MIB * ((cls + j) % 3) + ln, DEDUPS[(cls + j) % 3], comp))
    items += [(MIB, 1, 1), (2 * MIB, 2, 3), (3 * MIB, 3, (3, 2))]
    objs, total = _list(items, 0xA11C)
    count, zeros = class_counts(objs)
    assert all(count[c] >= 2 for c in range(FULL + 1))
    assert {c for c in RAGGED if zeros[c]} == {1, 3, 5, 7} and zeros[FULL]
    assert len({(o[3], o[4]) for o in objs}) >= 8
    return objs, total


def class_of_object(obj) -> int:
    """The class of the object's last chunk."""
    return chunk_class(obj[1] % MIB or MIB)


# ---- 4. several objects in one wave ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shared_wave(cls: int, knob: int):
    """64 / lpc + 3 objects with distinct tails of the class (one full wave of
    the class's launch and a partial one), or five where a chunk takes whole
    waves; compress mixed; two objects have full blocks in front.  The shortest
    tail of class 0 is 520 bytes, so every object has the sites the patterns use."""
    C = class_ceiling(cls)
    lo = 519 if cls == 0 else C // 2
    lpc, _lane = knob_lanes(cls, knob)
    n = 64 // lpc + 3 if lpc < 64 else 5
    lens = [lo + 1 + i * (_hi(cls) - lo - 1) // (n - 1) for i in range(n)]
    assert len(set(lens)) == n and lens[0] == lo + 1 and lens[-1] == _hi(cls)
    items = [(ln + (MIB if i == 1 else 2 * MIB if i == 3 else 0), DEDUPS[i % 3], COMPRESS[i % 4])
             for i, ln in enumerate(lens)]
    objs, total = _list(items, 0x5AA7E + 131 * cls + knob)
    _ragged(objs, cls)
    count, zeros = class_counts(objs)
    assert count[cls] == n and count[FULL] == 3 and 0 < zeros[cls] < n
    waves = -(-n * lpc // 64)
    assert waves >= 2 and (lpc >= 64 or (n * lpc) % 64)                  # a partial wave behind a full one
    return objs, total


def wave_objects(cls: int, knob: int) -> int:
    """Objects whose tails share the first wave of the class's launch."""
    lpc, _lane = knob_lanes(cls, knob)
    return max(1, 64 // lpc)


# ---- 5. large calls -----------------------------------------------------------------------------------

def remap_groups(nchunks: int, lpc: int, zeros: bool):
    """(full ks_remap groups, workgroups of the partial one) of a fill launch:
    a group is 8 XCDs x 16 one-wave workgroups, or with zero prefixes 8 x 8
    four-wave ones."""
    waves = -(-nchunks * lpc // 64)
    wgs, group = (-(-waves // 4), 64) if zeros else (waves, 128)
    return wgs // group, wgs % group


@functools.lru_cache(maxsize=None)
def many_tiny(n: int = 20000, zeros: bool = True):
    """n objects of 1 .. 80 bytes; with `zeros` every third of at least 2 bytes
    at compress 2, so the class-0 launch has zero prefixes.  Gaps are 16 to 48
    bytes here, which keeps the buffer near 100 bytes per object."""
    rng = random.Random(0x71A1 + n)
    objs, end = [], 0
    for k in range(n):
        size = 1 + k % 80
        off = (end + 15) // 16 * 16 + 16 * rng.randint(1, 3)
        if off % 4096 == 0:
            off += 16
        objs.append((off, size, 0x71A1 + 1000003 * k, 1, 2 if zeros and k % 3 == 0 and size >= 2 else 1))
        end = off + size
    total = (end + 15) // 16 * 16 + 4112
    rng.shuffle(objs)
    count, z = class_counts(objs)
    assert count[0] == n and sum(count) == n and (z[0] >= n // 4 if zeros else z[0] == 0)
    assert object_bytes(objs) <= BUDGET and total < 128 * n + 8192
    if n >= 20000:
        assert n > 4096 * 1.25 and n > 1024                               # both record tables and the per-object array regrow
        # the default rule on a device of CUS compute units gives the fill two
        # lanes per chunk here and the verify one
        assert class_lanes(4096, n, CUS, 0, zeros, 64, False)[0] == 2
        assert class_lanes(4096, n, CUS, 0, zeros, 64, True)[0] == 1
        for lpc in (1, 2):
            full, part = remap_groups(n, lpc, zeros)
            # one lane per chunk in four-wave workgroups (a knob that is set): 79 workgroups, one full group
            assert full >= (1 if zeros and lpc == 1 else 2) and part > 0, (lpc, full, part)
    return objs, total
