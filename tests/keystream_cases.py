"""Cases for the uniform keystream launches (k_keystream: xoshiro_fill,
dgen_fill, dgen_fill_stream), aimed at the places where
they can go wrong, and a plain restatement of their plan
(csrc/s3dg_ks_plan.h) that says where those places are.  No torch, no GPU:
tests/test_ks_plan_cpu.py holds the restatement against the header line by
line (tests/capi/ks_plan_table.cpp) and calls every builder at 256 and 304
compute units, so each builder's own coverage assertions run in the CPU
suite; tests/test_gpu_keystream_edges.py runs the cases on a device with the
device's own CU count.  Not a conftest.

Every builder takes `cus`; counts that depend on it are derived.  A knob of 0
means "not set by the caller" (the library then holds 2048).
"""
from __future__ import annotations

import functools

MIB = 1 << 20
GRANULE = 4096
DEFAULT_DRAWS = 2048              # kDefaultKsMinDraws, both modes
LONG_DRAWS, LONG_ROUNDS = 4096, 4
MIN_SPAN = 256
PREFIX_DRAWS = 512
MAX_LPC = 1024
PERSIST_ROUNDS = 6
DRAWS = (16, 32, 64)              # stage widths D
WAVES = (1, 4)
M64 = (1 << 64) - 1
PHI = 0x9E3779B97F4A7C15


# ---- the plan, restated from the header's comments ---------------------------------------------

def lanes(mode, chunk_bytes, nchunks, zero_prefix, z0, knob, D, cus):
    """(lpc, span, ok).  mode 0 K2, 1 DG1; z0 > 0: a split's tails."""
    nd = chunk_bytes // 8 - z0
    m = knob or DEFAULT_DRAWS
    if mode == 1 and zero_prefix and m == DEFAULT_DRAWS:
        m = PREFIX_DRAWS
    if mode == 0 and m == DEFAULT_DRAWS and nd >= 64 * LONG_DRAWS:
        if nchunks * (nd // LONG_DRAWS) // 64 >= LONG_ROUNDS * cus * 4:
            m = LONG_DRAWS
    lpc = 1
    while lpc < MAX_LPC and nd // (2 * lpc) >= m:
        lpc *= 2
    if z0 and lpc < 64 and nd >= 64 * MIN_SPAN:
        lpc = 64
    while lpc < MAX_LPC and nchunks * lpc < cus * 4 * 64 and nd // (2 * lpc) >= MIN_SPAN:
        lpc *= 2
    span = -(-nd // lpc)
    span = -(-span // D) * D
    return lpc, span, span <= 0xFFFFFFFF


def lane_region(clen, z0, span, sub):
    """(rb, rlen) of lane `sub` of a chunk of clen bytes; rlen 0: nothing."""
    rb = (z0 + sub * span) * 8
    return rb, max(0, min(clen - rb, span * 8))


def dgen_call(obj_size, n_objs, lo, hi, f_num, f_den, split):
    """(zw, cut_last, zsplit, nchunks, z0) of blocks [lo, hi), hi clipped."""
    nb = -(-obj_size // MIB)
    nchunks = (hi - lo) * n_objs
    zw = (MIB * f_num // f_den) & ~(GRANULE - 1)
    ragged = obj_size % MIB != 0 and hi == nb
    ok = f_num > 0 and split > 0 and zw >= 8 * GRANULE
    cut = ok and ragged and hi - 1 > lo and (hi - 1 - lo) * n_objs >= split
    zsplit = ok and not ragged and nchunks >= split
    return zw, cut, zsplit, nchunks, (zw // 8 if zsplit else 0)


def half_tail(tail, res, cus, waves, D, n_objs, nchunks, chunk0, lpc, span):
    """None, or (T, lpc2, span2, chunk0_2, doff, cpo2, nchunks1, cpo1)."""
    T = res * cus * waves * 64 // lpc // 2 if tail < 0 else tail
    s2 = span // 2
    if not (n_objs == 1 and T > 0 and waves == 1 and 64 <= lpc <= 512 and s2 >= MIN_SPAN and s2 % D == 0
            and nchunks >= 8 * T):
        return None
    return T, 2 * lpc, s2, chunk0 + nchunks - T, (nchunks - T) * MIB, T, nchunks - T, nchunks - T


def static_grid(nchunks, lpc, waves, xcd_waves):
    """(wgs, nwg as the kernel sees it, xg)."""
    wgs = -(-(-(-nchunks * lpc // 64)) // waves)
    return wgs, min(wgs, 0x7FFFFFFF), (xcd_waves // waves if xcd_waves > waves else 1)


def persistent_grid(wgs, wgs2, rounds, res, cus, waves):
    """Workgroups of the persistent grid, 0: static."""
    r = (PERSIST_ROUNDS if waves == 1 else 0) if rounds < 0 else rounds
    cap = res * cus // 8 * 8
    return cap if r and cap >= 8 and wgs + wgs2 >= r * cap else 0


def remap(xg, nwg, b):
    if xg > 1 and (b // (8 * xg) + 1) * 8 * xg <= nwg:
        x, k = b % 8, b // 8
        return k // xg * 8 * xg + x * xg + k % xg
    return b


def quota(nwg, v, W):
    return W * ((nwg + 7 - v) // 8)


def fastmod_magic(d):
    return (M64 // d + 1) & M64


def fastmod(a, M, d):
    return (((M * a) & M64) * d) >> 64


def table_lines():
    """tests/capi/ks_plan_table.cpp's output, from the restatement."""
    out = []
    chunks = (128, 2176, 4096, 65664, MIB - 128, MIB, 2 * MIB + 128, 4202496, 16 * MIB, 64 * MIB)
    knobs = (0, 64, 256, 512, 2048, 4096, 131072)
    ncs = (1, 3, 33, 700, 1 << 20)
    cuss = (1, 256, 304)
    for cb in chunks:
        for knob in knobs:
            for nc in ncs:
                for cus in cuss:
                    for D in DRAWS:
                        lpc, span, ok = lanes(0, cb, nc, False, 0, knob, D, cus)
                        out.append(f"lanes 0 {cb} {nc} 0 0 {knob} {D} {cus} {lpc} {span} {int(ok)}")
    ratios = ((0, 1), (1, 2), (2, 3), (1, 3), (6, 7), (19, 20), (99, 100), (127, 128), (65534, 65535))
    for fn, fd in ratios:
        for knob in knobs:
            for nc in ncs:
                for cus in cuss:
                    for D in DRAWS:
                        for split in (0, 1):
                            _zw, _cut, zs, _n, z0 = dgen_call(nc * MIB, 1, 0, nc, fn, fd, split)
                            zp = fn > 0 and not zs
                            lpc, span, ok = lanes(1, MIB, nc, zp, z0, knob, D, cus)
                            out.append(f"lanes 1 {MIB} {nc} {int(zp)} {z0} {knob} {D} {cus} {lpc} {span} {int(ok)}")
    for z0 in (0, 87040, 129536):
        for span in (272, 320, 352, 384, 2048):
            for clen in (1, 65664, MIB - 3, MIB):
                for sub in (0, 1, 2, 30, 31, 63, 125, 127, 255, 1023):
                    rb, rlen = lane_region(clen, z0, span, sub)
                    out.append(f"region {clen} {z0} {span} {sub} {rb} {rlen}")
    for size in (MIB, 2 * MIB, 2 * MIB + 5, 5 * MIB, 5 * MIB + 4095, 64 * MIB, 65 * MIB + 1):
        for n_objs in (1, 3):
            for fn, fd in ratios:
                for split in (0, 1, 2, 64):
                    nb = -(-size // MIB)
                    for lo in (0, 1):
                        for hi in (nb, nb - 1):
                            if lo >= hi:
                                continue
                            zw, cut, zs, n, z0 = dgen_call(size, n_objs, lo, hi, fn, fd, split)
                            out.append(f"call {size} {n_objs} {lo} {hi} {fn} {fd} {split} {zw} {int(cut)} {int(zs)} {n} {z0}")
    for tail in (-1, 0, 1, 3, 32, 1000):
        for res in (0, 1, 8):
            for cus in cuss:
                for waves in (1, 4):
                    for D in DRAWS:
                        for n_objs in (1, 2):
                            for nc in (7, 24, 256, 6145):
                                for lpc in (32, 64, 256, 512, 1024):
                                    for span in (352, 512, 544, 2048):
                                        H = half_tail(tail, res, cus, waves, D, n_objs, nc, 5, lpc, span)
                                        h = " ".join(str(x) for x in H) if H else "0 0 0 0 0 0 0 0"
                                        out.append(f"tail {tail} {res} {cus} {waves} {D} {n_objs} {nc} {lpc} {span} "
                                                   f"{int(H is not None)} {h}")
    for nc in (1, 3, 33, 257, 1 << 20, 1 << 40):
        for lpc in (1, 2, 32, 64, 512, 1024):
            for waves in (1, 2, 4):
                for xcd in (1, 4, 16, 32, 4096):
                    wgs, nwg, xg = static_grid(nc, lpc, waves, xcd)
                    out.append(f"grid {nc} {lpc} {waves} {xcd} {wgs} {nwg} {xg}")
    for wgs in (7, 255, 256, 1535, 1536, 100000):
        for wgs2 in (0, 1, 64):
            for rounds in (-1, 0, 1, 3, 6):
                for res in (0, 1, 3, 8):
                    for cus in (0, 1, 7, 8, 256, 304):
                        for waves in (1, 2, 4):
                            out.append(f"persist {wgs} {wgs2} {rounds} {res} {cus} {waves} "
                                       f"{persistent_grid(wgs, wgs2, rounds, res, cus, waves)}")
    for xg in (1, 2, 4, 16):
        for nwg in (1, 7, 8, 33, 64, 129, 300):
            for b in range(nwg):
                out.append(f"remap {xg} {nwg} {b} {remap(xg, nwg, b)}")
    for nwg in (0, 1, 7, 8, 9, 33, 0x7FFFFFFF):
        for v in range(8):
            for W in (1, 2, 4):
                out.append(f"quota {nwg} {v} {W} {quota(nwg, v, W)}")
    for U in (1, 3, 65537, 0xFFFFFFFF):
        for a in (0, 1, 2, 65536, 65537, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF):
            out.append(f"fastmod {a} {U} {fastmod_magic(U)} {fastmod(a, fastmod_magic(U), U)}")
    return out


# ---- what a launch looks like ---------------------------------------------------------------------

def lane_stats(clen, z0, lpc, span):
    """(full lanes, draws of the partial lane or 0, empty lanes) of one chunk;
    the regions tile [8 z0, clen) exactly once."""
    full = part = empty = 0
    at = 8 * z0
    for sub in range(lpc):
        rb, rlen = lane_region(clen, z0, span, sub)
        if rlen == span * 8:
            full += 1
        elif rlen:
            assert part == 0
            part = -(-rlen // 8)
        else:
            empty += 1
        if rlen:
            assert rb == at and rb + rlen <= clen
            at += rlen
    assert at == max(clen, 8 * z0) and full + (part > 0) + empty == lpc
    return full, part, empty


def ratio_of(compress):
    """(f_num, f_den) of a compress value given as an int or a (num, den) pair,
    as s3dlio_amd.compress_ratio (held equal in tests/test_ks_plan_cpu.py)."""
    from fractions import Fraction
    fr = Fraction(*compress) if isinstance(compress, tuple) else Fraction(compress)
    return (0, 1) if fr <= 1 else (fr.numerator - fr.denominator, fr.numerator)


def compress_of(f_num, f_den):
    """The compress value whose ratio is f_num / f_den (in lowest terms)."""
    from math import gcd
    g = gcd(f_num, f_den)
    return (f_den // g, (f_den - f_num) // g)


def dgen_launches(cus, size, n_objs=1, lo=0, hi=None, compress=1, split=64, knob=0, D=64, waves=0, xcd=0,
                  persist=-1, tail=0, res=1):
    """The keystream launches of one DG1 call, in order: dicts with z0, lpc,
    span, nchunks, chunk0, waves, xg, nwg, grid (0: static), jump ('none',
    'scalar' or 'vector'), and 'A2' (a dict of the same, or None).  waves /
    xcd 0: not set by the caller; res: resident workgroups per CU of the shape
    (query_keystream_occupancy)."""
    fn, fd = ratio_of(compress)
    nb = -(-size // MIB)
    hi = nb if hi is None else min(hi, nb)
    if lo >= hi or n_objs == 0:
        return []
    zw, cut, zs, nchunks, z0 = dgen_call(size, n_objs, lo, hi, fn, fd, split)
    kw = dict(compress=compress, split=split, knob=knob, D=D, waves=waves, xcd=xcd, persist=persist, tail=tail, res=res)
    if cut:
        return dgen_launches(cus, size, n_objs, lo, hi - 1, **kw) + dgen_launches(cus, size, n_objs, hi - 1, hi, **kw)
    zp = fn > 0 and not zs
    lpc, span, ok = lanes(1, MIB, nchunks, zp, z0, knob, D, cus)
    assert ok
    W = waves or (4 if zp else 1)
    xw = xcd or (32 if zp else 16)
    n1, A2 = nchunks, None
    H = half_tail(tail, res, cus, W, D, n_objs, nchunks, lo, lpc, span)
    if H:
        T, lpc2, span2, c0, doff, _cpo2, n1, _cpo1 = H
        wgs2, nwg2, xg2 = static_grid(T, lpc2, W, xw)
        A2 = dict(z0=z0, lpc=lpc2, span=span2, nchunks=T, chunk0=c0, doff=doff, nwg=nwg2, xg=xg2, wgs=wgs2)
    wgs, nwg, xg = static_grid(n1, lpc, W, xw)
    grid = persistent_grid(wgs, A2["wgs"] if A2 else 0, persist, res, cus, W)
    jump = "scalar" if lpc >= 64 else "vector" if (z0 or lpc > 1) else "none"
    return [dict(z0=z0, zw=zw if zs else 0, lpc=lpc, span=span, nchunks=n1, chunk0=lo, waves=W, xg=xg, nwg=nwg,
                 wgs=wgs, grid=grid, jump=jump, A2=A2, zero_prefix=zp)]


def k2_launch(cus, chunk, nchunks, knob=0, D=64, waves=1, xcd=16, persist=-1, res=1):
    lpc, span, ok = lanes(0, chunk, nchunks, False, 0, knob, D, cus)
    assert ok
    wgs, nwg, xg = static_grid(nchunks, lpc, waves, xcd)
    return dict(z0=0, lpc=lpc, span=span, nchunks=nchunks, waves=waves, xg=xg, nwg=nwg, wgs=wgs,
                grid=persistent_grid(wgs, 0, persist, res, cus, waves),
                jump="scalar" if lpc >= 64 else "vector" if lpc > 1 else "none")


# ---- (a) K2 lane geometry ------------------------------------------------------------------------------

# the issue's table at 256 CUs: (chunk bytes, D) -> (lanes, span, full, partial draws, empty)
K2_TABLE = {
    (65664, 16): (32, 272, 30, 48, 1),
    (65664, 64): (32, 320, 25, 208, 6),
    (2 * MIB + 128, 64): (1024, 320, 819, 80, 204),
    (4202496, 64): (1024, 576, 912, 0, 112),
}
K2_BIG = (16 * MIB, 64 * MIB)     # one chunk each: spans of 2048 and 8192 draws


def k2_chunk_for(lpc: int) -> int:
    """A chunk size (a multiple of 128) that a launch of 1 or 3 chunks gives
    `lpc` lanes, with a ragged last lane: 256 lpc + 16 draws."""
    return 2048 * lpc + 128


@functools.lru_cache(maxsize=None)
def k2_geometry(cus: int):
    """Chunk sizes for launches of 1 and 3 chunks: the table's, one per lpc
    1 .. 1024, and (one chunk only) 16 MiB and 64 MiB."""
    sizes = [65664, 2 * MIB + 128, 4202496]
    for (chunk, D), want in K2_TABLE.items():
        lpc, span, _ok = lanes(0, chunk, 1, False, 0, 0, D, cus)
        assert (lpc, span) + lane_stats(chunk, 0, lpc, span) == want, (chunk, D)
    seen = set()
    k = 1
    while k <= MAX_LPC:
        chunk = k2_chunk_for(k)
        for n in (1, 3):
            for D in DRAWS:
                lpc, span, _ok = lanes(0, chunk, n, False, 0, 0, D, cus)
                assert lpc == k, (k, n, D, lpc)
                full, part, empty = lane_stats(chunk, 0, lpc, span)
                assert part or empty or k == 1                      # a ragged or an empty last lane
        seen.add(k)
        if chunk not in sizes:
            sizes.append(chunk)
        k *= 2
    assert seen == {1 << j for j in range(11)}
    for chunk, want in zip(K2_BIG, (2048, 8192)):
        for D in DRAWS:
            assert lanes(0, chunk, 1, False, 0, 0, D, cus)[:2] == (1024, want)
            assert want // D >= 32                                      # many stages per lane
    # the unit's jump path: none at one lane, per lane below 64, on the scalar unit from 64
    assert {k2_launch(cus, c, 1)["jump"] for c in sizes} == {"none", "vector", "scalar"}
    return tuple(sizes)


def k2_boundaries(cus: int, chunk: int, nchunks: int, D: int):
    """Three lane boundaries of the last chunk (byte offsets): the first, a
    middle one and the start of the last lane that has bytes; with one lane:
    stage boundaries."""
    lpc, span, _ok = lanes(0, chunk, nchunks, False, 0, 0, D, cus)
    step = span * 8 if lpc > 1 else D * 8
    nb = (chunk - 1) // step                                            # boundaries inside the chunk
    assert nb >= 1, (chunk, lpc, span)
    return sorted({step, step * ((nb + 1) // 2), step * nb})


def k2_cuts(cus: int, chunk: int, nchunks: int, D: int):
    """Lengths of the last chunk: the whole chunk and 17 bytes to either side
    of k2_boundaries.  So the 1 .. 7 byte tail draw is a lane's first draw
    (b + t) and a lane's last (b - 8 + t) for every t, with the high-half
    (1 .. 4) and low-half (5 .. 7) forms."""
    bs = k2_boundaries(cus, chunk, nchunks, D)
    cuts = {chunk}
    for b in bs:
        cuts |= {b + d for d in range(-17, 18) if 1 <= b + d <= chunk}
    first, last = set(), set()
    for b in bs:
        for t in range(1, 9):
            assert b - 8 + t in cuts
            last.add(t)
            if b + t <= chunk:
                first.add(t)
    assert last == set(range(1, 9)) and first == set(range(1, 9)), (chunk, D)
    return sorted(cuts)


# ---- (b) DG1 zero-split tails ---------------------------------------------------------------------------

def _candidates():
    """Ratios n / (n + 1) for n <= 128, then wide denominators."""
    for n in range(1, 129):
        yield n, n + 1
    for d in (256, 4096, 65535, 65536, 1000003):
        for n in range(d // 2, d):
            yield n, d


def _find(pred, what):
    for fn, fd in _candidates():
        if MIB * fn // fd // GRANULE >= 8 and pred(fn, fd):
            return fn, fd
    raise AssertionError(f"no ratio gives {what}")


def tail_lanes(cus, fn, fd, nchunks, D):
    """(lpc, span, z0) of the tail launch of a split of nchunks full blocks."""
    zw, _cut, zs, _n, z0 = dgen_call(nchunks * MIB, 1, 0, nchunks, fn, fd, 1)
    assert zs and z0 == zw // 8
    lpc, span, _ok = lanes(1, MIB, nchunks, False, z0, 0, D, cus)
    return lpc, span, z0


# the issue's table at 256 CUs: (ratio, D) -> (z0, lanes, span, full, partial draws, empty)
SPLIT_TABLE = {
    ((2, 3), 16): (87040, 128, 352, 125, 32, 2),
    ((2, 3), 64): (87040, 128, 384, 114, 256, 13),
    ((1, 3), 64): (43520, 256, 384, 228, 0, 28),
}
SPLIT_BLOCKS = (2, 5, 6)          # blocks per launch: objects of 2 and of 5, a stream of 3 objects of 2


@functools.lru_cache(maxsize=None)
def split_ratios(cus: int):
    """{name: (f_num, f_den)} for launches of 2, 5 and 6 full blocks with a
    split threshold of 1: tails of 2, 4, 16 and 32 lanes (the per-lane jump
    with z0 > 0, taken by lane 0 too), 64 lanes forced by the tail rule, 128
    and 256 lanes, and a remainder zlen - zw of every value 0 .. 15 and of
    4080 bytes."""
    out = {}

    def every(fn, fd, pred):
        return all(pred(*tail_lanes(cus, fn, fd, n, D)) for n in SPLIT_BLOCKS for D in DRAWS)

    for want in (2, 4, 16, 32, 128, 256):
        out[f"lanes{want}"] = _find(lambda fn, fd: every(fn, fd, lambda lpc, span, z0: lpc == want), f"{want} lanes")
    # 64 lanes because the tail rule forces them: the knob's rule alone gives fewer
    def forced(fn, fd):
        def one(lpc, span, z0):
            nd = MIB // 8 - z0
            by_knob = 1
            while by_knob < MAX_LPC and nd // (2 * by_knob) >= DEFAULT_DRAWS:
                by_knob *= 2
            return lpc == 64 and by_knob < 64 and nd >= 64 * MIN_SPAN
        return every(fn, fd, one)
    out["lanes64"] = _find(forced, "64 forced lanes")
    for rem in list(range(16)) + [4080]:
        out[f"rem{rem}"] = _find(lambda fn, fd: MIB * fn // fd % GRANULE == rem, f"a remainder of {rem}")
    out["c3"], out["c3/2"] = (2, 3), (1, 3)
    # what the list is built for
    for name, (fn, fd) in out.items():
        assert 0 < fn < fd and ratio_of(compress_of(fn, fd)) == (fn // _g(fn, fd), fd // _g(fn, fd))
        for n in SPLIT_BLOCKS:
            for D in DRAWS:
                L = dgen_launches(cus, n * MIB, compress=compress_of(fn, fd), split=1, D=D)
                assert len(L) == 1 and L[0]["z0"] > 0 and not L[0]["zero_prefix"]
                if name in ("lanes2", "lanes4", "lanes16", "lanes32"):
                    assert L[0]["jump"] == "vector" and L[0]["lpc"] < 64
                U = dgen_launches(cus, n * MIB, compress=compress_of(fn, fd), split=0, D=D)
                assert len(U) == 1 and U[0]["z0"] == 0 and U[0]["zero_prefix"] and U[0]["waves"] == 4
    rems = {MIB * fn // fd % GRANULE for fn, fd in out.values()}
    assert set(range(16)) | {4080} <= rems and {r % 16 for r in rems} == set(range(16))
    for (r, D), want in SPLIT_TABLE.items():
        lpc, span, z0 = tail_lanes(cus, *r, 2, D)
        assert (z0, lpc, span) + lane_stats(MIB, z0, lpc, span) == want, (r, D)
    parts = set()
    for fn, fd in out.values():
        for D in DRAWS:
            lpc, span, z0 = tail_lanes(cus, fn, fd, 2, D)
            full, part, empty = lane_stats(MIB, z0, lpc, span)
            parts.add((part > 0, empty > 0))
    assert {(True, True), (False, True), (False, False)} <= parts        # partial + empty, empty alone, neither
    return out


def _g(a, b):
    from math import gcd
    return gcd(a, b)


def ragged_split(cus: int, size: int, n_objs: int, compress, D: int):
    """A ragged object with a threshold of 1: its full blocks split, the
    ragged last block in a call of its own; the block range that ends before
    the last block splits too."""
    nb = -(-size // MIB)
    assert size % MIB and nb >= 2
    L = dgen_launches(cus, size, n_objs, compress=compress, split=1, D=D)
    assert len(L) == 2 and L[0]["z0"] > 0 and L[0]["nchunks"] == (nb - 1) * n_objs
    assert L[1]["z0"] == 0 and L[1]["zero_prefix"] and L[1]["nchunks"] == n_objs and L[1]["chunk0"] == nb - 1
    R = dgen_launches(cus, size, 1, 0, nb - 1, compress=compress, split=1, D=D)
    assert len(R) == 1 and R[0]["z0"] > 0 and R[0]["nchunks"] == nb - 1
    return L


# ---- (c) DG1 long lanes ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def late_prefix():
    """A ratio whose zero prefix ends inside a stage (and inside a 16-byte
    piece) in the last quarter of the stages of its lane, for lanes of 512 and
    of 1024 draws alike."""
    fn, fd = _find(lambda fn, fd: MIB * fn // fd % 8192 >= 7168 and MIB * fn // fd % 512 and MIB * fn // fd % 16,
                   "a prefix that ends in a late stage")
    return compress_of(fn, fd)


def long_lanes(cus: int, draws: int, prefix: bool = False):
    """(size, knob, compress) of one object whose lanes are `draws` long (512,
    1024 or 2048): at least cus * 256 lanes, so the small-launch spread leaves
    them alone, and a ragged end with a 3-byte tail.  prefix: a zero prefix
    inside the lanes (no split) that ends mid-stage in the last quarter of its
    lane's stages; with the knob not set the library plans 512-draw lanes for
    a prefix, so 2048-draw lanes (knob "not set") exist at compress 1 only."""
    assert not (prefix and draws == DEFAULT_DRAWS)
    compress = late_prefix() if prefix else 1
    lpc = MIB // 8 // draws
    nchunks = -(-cus * 256 // lpc)
    knob = 0 if draws == DEFAULT_DRAWS else draws
    size = nchunks * MIB + MIB // 2 + 8 * 1237 + 3
    L = dgen_launches(cus, size, compress=compress, split=0, knob=knob, D=64)
    assert len(L) == 1
    assert (L[0]["lpc"], L[0]["span"]) == (lpc, draws), (draws, compress, L[0])
    # one chunk fewer and the spread would have halved the lanes
    assert lanes(1, MIB, nchunks - 1, prefix, 0, knob, 64, cus)[0] == 2 * lpc or nchunks * lpc > cus * 256
    assert size % 8 == 3 and size % MIB
    if prefix:
        fn, fd = ratio_of(compress)
        zlen = MIB * fn // fd
        span_b = draws * 8
        stages = span_b // 512
        assert zlen % 512 and zlen % span_b // 512 >= stages * 3 // 4, (zlen, span_b)
        assert lanes(1, MIB, nchunks, True, 0, 0, 64, cus)[:2] == (256, 512)   # what an unset knob would give
    return size, knob, compress


# ---- (d) the persistent grid at small shapes -------------------------------------------------------------

def persistent_dgen(cus: int, res: int, waves: int, xcd: int, D: int = 64):
    """(chunks, launch) of a DG1 object at 512 lanes per chunk (knob 256) on a
    persistent grid of res * cus workgroups (rounds = 1): the fewest chunks
    that make it persistent, plus one (33 at 256 CUs, 1-wave workgroups, a
    cap of 1 per CU), so the queues are of unequal length."""
    cap = res * cus // 8 * 8
    n = -(-cap * waves * 64 // 512) + 1
    L = dgen_launches(cus, n * MIB, split=0, knob=256, D=D, waves=waves, xcd=xcd, persist=1, res=res)[0]
    assert L["lpc"] == 512 and L["grid"] == cap and L["nwg"] >= cap
    # a chunk is 8 waves: with 1-wave workgroups the queues are equal, with 2 and 4 waves one chunk
    # beyond a multiple of the cap leaves them unequal
    assert waves == 1 or len({quota(L["nwg"], v, waves) for v in range(8)}) == 2
    return n, L


def persistent_k2(cus: int, res: int, waves: int, xcd: int, rem: int, chunk: int = 65664, D: int = 64):
    """(chunks, launch) of a K2 launch of 65 664-byte chunks on the persistent
    grid with nwg % 8 == rem."""
    n = 1
    while True:
        L = k2_launch(cus, chunk, n, D=D, waves=waves, xcd=xcd, persist=1, res=res)
        if L["grid"] and L["nwg"] % 8 == rem and (L["xg"] == 1 or L["nwg"] % (8 * L["xg"])):
            break
        n += 1
        assert n < 1 << 16
    if L["xg"] > 1:
        assert L["nwg"] >= 8 * L["xg"] and L["nwg"] % (8 * L["xg"])     # full remap groups and a partial last one
    full, part, empty = lane_stats(chunk, 0, L["lpc"], L["span"])
    assert part or empty
    return n, L


# ---- (e) the half-length tail set ---------------------------------------------------------------------------

def half_tail_object(cus: int, res: int, T: int, persist: int, ragged: bool, lpc: int = 256, D: int = 64):
    """(size, knob, launch): one object of `lpc` lanes per chunk whose last T
    chunks run as a second set of lanes half as long; persist 1: both sets in
    one persistent launch (res: the shape's resident workgroups per CU);
    persist 0: A2 as a second static launch."""
    knob = MIB // 8 // lpc
    nchunks = max(-(-cus * 256 // lpc), 8 * T)
    size = nchunks * MIB - ((MIB // 3 + 5) if ragged else 0)
    L = dgen_launches(cus, size, split=0, knob=knob, D=D, waves=1, persist=persist, tail=T, res=res)
    assert len(L) == 1
    L = L[0]
    A2 = L["A2"]
    assert (L["lpc"], L["span"]) == (lpc, knob) and A2 is not None, L
    assert (A2["lpc"], A2["span"], A2["nchunks"]) == (2 * lpc, knob // 2, T)
    assert L["nchunks"] + T == nchunks and A2["chunk0"] == L["nchunks"] and A2["doff"] == L["nchunks"] * MIB
    assert bool(L["grid"]) == bool(persist), L
    return size, knob, L


# ---- (f) block indices near 2^32 -------------------------------------------------------------------------------

FAR_BLOCKS = (1 << 32) - 1        # the most blocks an object may have
FAR_RANGES = ((0, 2), ((1 << 31) - 1, (1 << 31) + 1), ((1 << 32) - 3, (1 << 32) - 1), ((1 << 32) - 2, 1 << 32))


def far_seed(seed: int, i: int, U: int) -> int:
    """Seed input of block i of an object with U unique blocks: the header's definition."""
    return seed ^ ((i % U) * PHI & M64)
